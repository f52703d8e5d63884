"""Boxes, blends and oracle chains of tests/test_gpu_update_classes.py and
tests/test_update_classes_host.py: one box per edge of every size class of the register-resident
update kernels (csrc/common.h: kUpdateNpl x kUpdateTeam), of every sweep plan they can take and of
the general kernel.  Nothing here needs a GPU.

A blend holds ONE component on a two-band 128 x 128 plane, so a component's gradient depends on
nothing else and a blend stepped alone has the same bits to show as in any batch.
"""

from collections import namedtuple

import numpy as np

C, H, W = 2, 128, 128
NOISE = np.array([0.02, 0.03], dtype=np.float32)

# csrc/common.h, restated.  If these move, the table below has to be revisited: its rows are
# chosen for the edges of THESE classes (tests/test_update_classes_host.py says so when it fails).
UPDATE_NPL = (7, 16, 27, 42, 59, 16, 27, 42, 59)
UPDATE_TEAM = (64, 64, 64, 64, 64, 256, 256, 256, 256)
MAX_REGISTER_BOX = 256 * 59
NUM_SMALL_CLASSES = 5
FAST_SLOT_PIXELS = 16376  # csrc/batch.hip: the slot layout of a sweep plan (16-bit LDS addresses)
GENERAL = -1  # "class" of a box beyond MAX_REGISTER_BOX: the general update kernel


def update_class(n_pix):
    for c, (npl, team) in enumerate(zip(UPDATE_NPL, UPDATE_TEAM)):
        if n_pix <= npl * team:
            return c
    return GENERAL


# The sweep a box takes inside the update kernels (launch_update / update_component in
# csrc/kernels.hip, refresh_view in csrc/batch.hip):
#   RING       centred odd square up to 47^2 in a one-wavefront class: the one-plane ring schedule
#   RING_LATE  the same from 49^2 on: rings 24 .. 31 start late
#   LEVEL      everything else: the level plan in its slot layout -- oblong and even boxes, every
#              four-wavefront class (63^2 has a one-plane ring schedule but a team of four), the
#              two-plane radii from 65^2 on
#   LEVEL_NO_SLOTS  more than 16376 pixels: no slot layout, `fast_plans` off for the whole batch
RING, RING_LATE, LEVEL, LEVEL_NO_SLOTS = "ring", "ring_late", "level", "level_no_slots"

# (box shape, pixels, class, plan)
BOXES = [
    ((21, 21), 441, 0, RING),
    ((16, 28), 448, 0, LEVEL),           # class 0 full, even sides
    ((15, 30), 450, 1, LEVEL),           # first beyond class 0
    ((32, 32), 1024, 1, LEVEL),          # class 1 full
    ((25, 41), 1025, 2, LEVEL),          # first beyond class 1
    ((36, 48), 1728, 2, LEVEL),          # class 2 full
    ((37, 47), 1739, 3, LEVEL),          # 11 pixels into class 3
    ((47, 47), 2209, 3, RING),           # the last ring plan without late rings (ring 23)
    ((49, 49), 2401, 3, RING_LATE),      # the first with late rings (ring 24)
    ((48, 56), 2688, 3, LEVEL),          # class 3 full
    ((51, 53), 2703, 4, LEVEL),          # 15 pixels into class 4
    ((61, 61), 3721, 4, RING_LATE),
    ((59, 64), 3776, 4, LEVEL),          # class 4 full: the largest one-wavefront box
    ((60, 63), 3780, 5, LEVEL),          # 4 pixels into the first team class
    ((63, 63), 3969, 5, LEVEL),          # ring-eligible (ring 31), but a team of four
    ((64, 64), 4096, 5, LEVEL),          # class 5 full
    ((58, 71), 4118, 6, LEVEL),          # 22 pixels into class 6
    ((65, 65), 4225, 6, LEVEL),          # the first two-plane radius (ring 32)
    ((72, 96), 6912, 6, LEVEL),          # class 6 full
    ((83, 84), 6972, 7, LEVEL),          # 60 pixels into class 7
    ((101, 101), 10201, 7, LEVEL),
    ((96, 112), 10752, 7, LEVEL),        # class 7 full
    ((104, 104), 10816, 8, LEVEL),       # 64 pixels into class 8
    ((121, 121), 14641, 8, LEVEL),
    ((118, 128), 15104, 8, LEVEL),       # class 8 full = kMaxRegisterBox
    ((123, 123), 15129, GENERAL, LEVEL),         # first beyond kMaxRegisterBox
    ((127, 128), 16256, GENERAL, LEVEL),         # the fast slots still fit
    ((128, 128), 16384, GENERAL, LEVEL_NO_SLOTS),  # 16384 > 16376
]
# one copy each of these hangs over the top and left edges of a frame smaller than the box, at a
# negative origin: the lane-by-lane gather (classes 0, 3, 5 and 7)
OVERHANG = [(21, 21), (49, 49), (63, 63), (101, 101)]
OVERHANG_ORIGIN = (-7, -5)
# Noise seed of a box's starting image where the default seed does not meet the conditions of
# tests/test_update_classes_host.py: the chain must have work to do, and the scene must be well
# conditioned.  The latter failed for these eight: their starting image has a centre pixel below
# 0.5, the maximum normalisation then scales the outer pixels up by 1 / (centre candidate) in each
# of the ten proximal sub-iterations, and the oracle's own answer moves by up to 2e-4 between its
# float64 and its float32 moments -- such a scene cannot hold a float32 kernel to 1e-5.
SEEDS = {"36x48": 1036051, "59x64": 1059067, "64x64": 1064067, "83x84": 1083087,
         "118x128": 1118131, "49x49_over": 1049059, "63x63_over": 1063073, "128x128": 1128131}

Blend = namedtuple("Blend", "name shape origin frame cls plan seed")


def _blend(shape, cls, plan, overhang=False, tag=""):
    h, w = shape
    name = "%dx%d%s%s" % (h, w, "_over" if overhang else "", tag)
    if overhang:
        # rows / columns 0 .. h - 8 / w - 6 of the box lie on the frame, which ends 3 rows and
        # 3 columns behind the box: top and left overhang only
        origin, frame = OVERHANG_ORIGIN, (h - 4, w - 2)
    else:
        origin, frame = ((H - h) // 3, (W - w) // 2), (H, W)
    seed = SEEDS.get(name, 1000 * h + w + (7 if overhang else 0) + len(tag))
    return Blend(name, shape, origin, frame, cls, plan, seed)


def register_blends():
    """The whole table of register-resident boxes: 25 boxes, the 4 overhanging copies and one
    more 21^2 blend (so that class 0 has two items on the plain gather)."""
    out = [_blend(s, c, p) for s, _, c, p in BOXES if c != GENERAL]
    by_shape = {s: (c, p) for s, _, c, p in BOXES}
    out += [_blend(s, *by_shape[s], overhang=True) for s in OVERHANG]
    out.append(_blend((21, 21), 0, RING, tag="_b"))
    return out


def general_blends():
    return [_blend(s, c, p) for s, _, c, p in BOXES if c == GENERAL]


def one_wavefront(blends):
    return [b for b in blends if 0 <= b.cls < NUM_SMALL_CLASSES]


def _r2(shape):
    h, w = shape
    yy, xx = np.mgrid[:h, :w]
    return ((yy - h // 2) / (0.17 * h)) ** 2 + ((xx - w // 2) / (0.22 * w)) ** 2


def start_image(blend):
    """The construction of tests/test_gpu_update_chain.py: not monotonic, some negative pixels,
    the maximum away from 1."""
    rng = np.random.default_rng(blend.seed)
    r2 = _r2(blend.shape)
    m = (np.exp(-0.5 * r2) * (1 + 0.3 * rng.normal(0, 1, blend.shape)) - 0.02).astype(np.float32)
    m *= np.float32(0.8)
    return m


def start_spectrum(blend):
    rng = np.random.default_rng(blend.seed + 500000)
    return (1 + rng.random(C)).astype(np.float32)


def observation(blend, zero=False):
    """(data, weights) of the blend's 128 x 128 plane.  `zero`: all-zero weights -- every gradient
    is zero and an iteration's result is the proximal chain of the starting image.  Otherwise noise
    per band plus 1.2 x spectrum x a narrower Gaussian, weights 1 / noise^2; beyond the frame of an
    overhanging blend finite padding of weight 0."""
    if zero:
        return np.zeros((C, H, W), np.float32), np.zeros((C, H, W), np.float32)
    rng = np.random.default_rng(blend.seed + 900000)
    fh, fw = blend.frame
    data = np.full((C, H, W), 3.0, np.float32)
    weights = np.zeros((C, H, W), np.float32)
    data[:, :fh, :fw] = (rng.normal(0, 1, (C, fh, fw)) * NOISE[:, None, None]).astype(np.float32)
    weights[:, :fh, :fw] = (1 / NOISE ** 2)[:, None, None]
    (h, w), (oy, ox) = blend.shape, blend.origin
    truth = np.exp(-0.5 * _r2(blend.shape) * 1.3).astype(np.float32)
    ys, xs = slice(max(oy, 0), min(oy + h, fh)), slice(max(ox, 0), min(ox + w, fw))
    sed = start_spectrum(blend)
    data[:, ys, xs] += (1.2 * sed[:, None, None] * truth[None])[:, ys.start - oy:ys.stop - oy,
                                                                 xs.start - ox:xs.stop - ox]
    return data, weights


# ------------------------------------------------------------------ the chain alone (zero gradient)
# name -> scheme ("adam": AMSGrad of Blend.fit, kernel mode 0; "lite": lite's AdaProx, mode 1 -- the
# batch is lite as soon as a component fits its centre or has a background level; "fista": mode 2),
# weighting, min_gradient, links.  Links, in the order of the device chain: fit_center, bg
# (background threshold), symmetry strength, (l0 | l1, absolute threshold), positivity, centre-on
# floor, normalisation.
Chain = namedtuple("Chain", "scheme weighting min_gradient fit_center bg symmetry sparsity positive "
                            "cfloor norm")


def _chain(scheme="adam", weighting="angle", min_gradient=0.0, fit_center=False, bg=False,
           symmetry=None, sparsity=None, positive=True, cfloor=1e-6, norm=None):
    return Chain(scheme, weighting, min_gradient, fit_center, bg, symmetry, sparsity, positive,
                 cfloor, norm)


CHAINS = {
    # no normalisation: the device image is the oracle's chain bit for bit
    "no_norm": _chain(),
    "no_norm_fista": _chain(scheme="fista"),
    # lite's AdaProx needs a lite link: the fitted centre
    "no_norm_lite_fit_center": _chain(scheme="lite", fit_center=True),
    "flat_0.1": _chain(weighting="flat", min_gradient=0.1),
    "nearest": _chain(weighting="nearest"),
    "angle_0.25": _chain(min_gradient=0.25),
    "symmetry_1": _chain(symmetry=1.0),
    "symmetry_0.5": _chain(symmetry=0.5),
    "l0_absolute": _chain(sparsity=("l0", 0.05)),
    "l1_absolute": _chain(sparsity=("l1", 0.02)),
    # scarlet.lite's chain without its normalisation: fitted centre, background threshold in
    # the place of positivity, centre floor 1e-20
    "lite_bg_thresh": _chain(scheme="lite", fit_center=True, bg=True, positive=False, cfloor=1e-20),
    "norm_max": _chain(norm="max"),
    "norm_sum": _chain(norm="sum"),
}
BG_THRESH = 0.25
_OPERATORS = {}


def oracle_chain(x, chain, spectrum=None, upto_norm=False):
    """The oracle's chain (oracle.proxops, oracle.lite) of the float32 image `x`, once.
    `upto_norm`: stop in front of the normalisation."""
    from oracle import lite as olite
    from oracle import proxops

    x = np.array(x, dtype=np.float32)
    if chain.fit_center:
        # oracle.lite.monotonicity, with its operator kept per (shape, weighting, centre)
        h, w = x.shape
        centre = tuple(int(v) for v in olite.get_center(x, (h // 2, w // 2), 1))
        key = (x.shape, chain.weighting, centre)
        if key not in _OPERATORS:
            _OPERATORS[key] = proxops.monotonic_operator(x.shape, chain.weighting, centre)
        weights, didx, offsets = _OPERATORS[key]
        proxops.sweep(x, weights, offsets, didx, chain.min_gradient)
    else:
        x = proxops.prox_monotonic(x, 0, chain.weighting, chain.min_gradient)
    if chain.bg:  # lite/models.py:222-228 (oracle.lite.LiteComponent.prox_morph)
        level = NOISE * np.float32(BG_THRESH)
        model = spectrum[:, None, None] * x[None, :, :]
        x[np.all(model < level[:, None, None], axis=0)] = 0
    if chain.symmetry is not None:
        x = proxops.prox_soft_symmetry(x, 0, chain.symmetry)
    if chain.sparsity is not None:
        kind, thresh = chain.sparsity
        x = (proxops.prox_hard if kind == "l0" else proxops.prox_soft)(x, 0, thresh, "absolute")
    if chain.positive:
        x = proxops.prox_positivity(x, 0, np.float32(0))
    x = proxops.prox_center_on(x, 0, np.float32(chain.cfloor))
    assert x.dtype == np.float32
    if chain.norm is not None and not upto_norm:
        x = proxops.prox_normalization(x, 0, chain.norm)
    return x


def reciprocal_max_normalisation(u):
    """What the update kernels do for PROX_NORM_MAX ("one correctly rounded reciprocal per
    sub-iteration"): u * (1 / max) in float32, the maximum itself set to exactly 1."""
    u = np.asarray(u, dtype=np.float32)
    div = u.max()
    out = u * (np.float32(1) / div)
    out[u == div] = np.float32(1)
    assert out.dtype == np.float32
    return out


def ulp_distance(a, b):
    """Distance in units of the last place between finite float32 arrays of one sign."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def chain_spec_keywords(lib, chain):
    """ComponentSpec keywords (and BlendBatch keywords) of a chain of CHAINS."""
    flags = lib.PROX_MONOTONIC | lib.PROX_CENTER_ON
    flags |= lib.PROX_POSITIVE if chain.positive else 0
    flags |= lib.PROX_FIT_CENTER if chain.fit_center else 0
    flags |= lib.PROX_SYMMETRY if chain.symmetry is not None else 0
    flags |= {None: 0, "max": lib.PROX_NORM_MAX, "sum": lib.PROX_NORM_SUM}[chain.norm]
    kw = dict(neighbor_weight=chain.weighting, min_gradient=chain.min_gradient,
              center_floor=chain.cfloor)
    if chain.symmetry is not None:
        kw["sym_strength"] = chain.symmetry
    if chain.sparsity is not None:
        flags |= lib.PROX_L0 if chain.sparsity[0] == "l0" else lib.PROX_L1
        kw["l_thresh"] = chain.sparsity[1]
    if chain.bg:
        kw["bg_level"] = NOISE * np.float32(BG_THRESH)
    kw["prox_flags"] = flags
    batch_kw = {}
    if chain.scheme == "fista":
        kw["fista_step"] = float(1 / (2 * np.mean(1 / NOISE ** 2)))  # lite.init_fista_component
        batch_kw = dict(scheme="fista", log_norm=False)
    elif chain.scheme == "lite":
        kw["sed_min_step"] = NOISE / 10
        batch_kw = dict(log_norm=False)
    else:
        kw["sed_min_step"] = NOISE
    return kw, batch_kw


# ------------------------------------------------------------------ whole steps with a gradient
# name -> (ComponentSpec keywords without the flags, flag names, scheme, oracle keywords)
STEP_CASES = ["standard", "flat_symmetry_0.5", "nearest_l1_relative", "lite_adaprox", "lite_fista"]
N_STEPS = 3


def step_spec_keywords(lib, case):
    std = lib.PROX_EXTENDED_SOURCE
    lite_flags = lib.PROX_MONOTONIC | lib.PROX_FIT_CENTER | lib.PROX_CENTER_ON | lib.PROX_NORM_MAX
    lite_kw = dict(prox_flags=lite_flags, neighbor_weight="angle", min_gradient=0.0,
                   center_floor=1e-20, bg_level=NOISE * np.float32(BG_THRESH), morph_step=1e-2)
    if case == "standard":
        return dict(sed_min_step=NOISE), {}
    if case == "flat_symmetry_0.5":
        return dict(sed_min_step=NOISE, prox_flags=std | lib.PROX_SYMMETRY, neighbor_weight="flat",
                    min_gradient=0.1, sym_strength=0.5), {}
    if case == "nearest_l1_relative":
        # the thresholds of test_sparsity_constraints_and_center_floor
        return dict(sed_min_step=NOISE, prox_flags=std | lib.PROX_L1 | lib.PROX_L_RELATIVE,
                    neighbor_weight="nearest", min_gradient=0.0, l_thresh=3.0,
                    center_floor=1e-3), {}
    if case == "lite_adaprox":
        return dict(sed_min_step=NOISE / 10, **lite_kw), dict(log_norm=False)
    if case == "lite_fista":
        return (dict(fista_step=float(1 / (2 * np.mean(1 / NOISE ** 2))), **lite_kw),
                dict(scheme="fista", log_norm=False))
    raise KeyError(case)


PGM_KEYWORDS = {"standard": dict(),
                "flat_symmetry_0.5": dict(monotonic="flat", min_gradient=0.1, symmetric=0.5),
                "nearest_l1_relative": dict(monotonic="nearest", min_gradient=0.0,
                                            sparsity=("l1", 3.0, "relative"), tiny=1e-3)}


def oracle_steps(blend, case, state_dtype=np.float64):
    """The oracle's run of one blend: {"first": (sed, morph) after one iteration, "last": (sed,
    morph, v_morph or None) after N_STEPS, "loss": the losses, "log_norm": the constant in them
    (None: lite's loss, whose sign is the other way round)}.  `state_dtype=np.float32`: the
    oracle's restatement of float32 moments (oracle.pgm.Component), for the conditioning of the
    scene only -- the device is compared with the default."""
    from oracle import lite as olite
    from oracle import pgm

    data, weights = observation(blend)
    fh, fw = blend.frame
    data = np.ascontiguousarray(data[:, :fh, :fw])
    weights = np.ascontiguousarray(weights[:, :fh, :fw])
    sed, morph = start_spectrum(blend), start_image(blend)
    if case.startswith("lite_"):
        kind = case[5:]
        kw = (dict(fista_step=float(1 / (2 * np.mean(1 / NOISE ** 2)))) if kind == "fista"
              else dict(sed_min_step=NOISE / 10))
        comp = olite.LiteComponent(sed, morph, blend.origin, NOISE, bg_thresh=BG_THRESH, kind=kind,
                                   **kw)
        sc = olite.LiteScene(data, weights, None, [comp])
        sc.fit(1, e_rel=0, resize=None)
        first = (comp.sed.copy(), comp.morph.copy())
        sc.fit(N_STEPS, e_rel=0, resize=None)
        return dict(first=first, last=(comp.sed.copy(), comp.morph.copy(), None),
                    loss=np.array(sc.loss[:N_STEPS], dtype=np.float64), log_norm=None)
    comp = pgm.Component(sed, morph, blend.origin, sed_min_step=NOISE, state_dtype=state_dtype,
                         **PGM_KEYWORDS[case])
    sc = pgm.Scene(data.shape, data, weights, None, [comp])
    sc.step(0, 1e-3)
    first = (comp.sed.copy(), comp.morph.copy())
    for it in range(1, N_STEPS):
        sc.step(it, 1e-3)
    return dict(first=first, last=(comp.sed.copy(), comp.morph.copy(), comp.v_morph.copy()),
                loss=np.array(sc.loss, dtype=np.float64), log_norm=float(sc.log_norm))
