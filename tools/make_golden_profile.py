"""Golden vectors of the profile sources (GaussianSource, SpergelSource):
``tests/golden/profile_source.npz``.

BUILD-CONTAINER TOOLING (the reference checkout must be present):

    python tools/make_golden_profile.py

The reference is imported through ``oracle.refshim.load_reference`` (pattern of
``tools/make_golden_starlet.py``).  Scene: the quickstart scene ``hsc_cosmos_35`` with
``init_all_sources(max_components=1)``; the sources listed in ``PROFILES`` are replaced by
profile sources at the same catalogue positions -- a round Gaussian, a sheared one, one of sigma 6
whose box overhangs the frame, and a Spergel profile -- once on a float32 frame (construction,
model, rendering, logL) and once on a float64 frame (central finite differences of the
reference's own log-likelihood at two step sizes).  For ``nu`` the differences are taken with the
order of the reference's ``kv`` frozen at the current ``nu`` -- the rule its fit follows, since
``kv`` is registered without a derivative w.r.t. the order (morphology.py:380-381) -- and once
more unfrozen.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from oracle.refshim.load_reference import REFERENCE  # noqa: E402  (only names the checkout)
from make_golden_starlet import load_scarlet, save_deterministic  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
# source index -> ("gaussian", sigma, ellipticity) or ("spergel", nu, rhalf, ellipticity)
PROFILES = {
    0: ("gaussian", 1.5, (0.0, 0.0)),
    1: ("gaussian", 2.3, (0.2, -0.1)),
    3: ("gaussian", 6.0, (0.0, 0.0)),
    4: ("spergel", 0.5, 2.0, (0.1, 0.05)),
}
FD_H = 1e-3
GROUPS = ("center", "radius", "ellipticity", "nu")
SLOTS = {"center": slice(0, 2), "radius": slice(2, 3), "ellipticity": slice(3, 5), "nu": slice(5, 6)}
# (first centre, first radius, later centre, later radius) of the get_box / update() table
BOX_CASES = [
    ((20.2, 30.7), 1.5, (20.2, 30.7), 1.5),     # 15 -> 21 at the first hook
    ((20.2, 30.7), 2.3, (20.4, 30.6), 2.2),     # 23 -> 21
    ((20.2, 30.7), 6.0, (20.2, 30.7), 6.0),     # 60 -> 61
    ((20.2, 30.7), 2.1, (20.2, 30.7), 2.1),     # 21 -> 21: no change
    ((20.2, 30.7), 2.1, (20.2, 30.7), 2.1000001),  # just above 21: 31
    ((20.2, 30.7), 2.1, (20.6, 30.7), 2.1),     # the rounded centre moves
    ((20.5, 30.5), 2.1, (21.5, 31.5), 2.1),     # halves round to even
    ((20.2, 30.7), 3.1, (20.2, 30.7), 3.1),     # 31 -> 31
    ((20.2, 30.7), 3.1, (20.2, 30.7), 0.01),    # the smallest radius
    ((3.0, 2.0), 6.0, (-1.4, 50.2), 7.5),       # overhang on two edges, 81
]


def build(scarlet, dtype):
    from scarlet.initialization import init_all_sources

    d = np.load(os.path.join(REFERENCE, "data", "hsc_cosmos_35.npz"))
    images, psfs = d["images"], d["psfs"]
    filters = [str(f) for f in d["filters"]]
    weights = 1 / d["variance"]
    centers = [(s["y"], s["x"]) for s in d["catalog"]]
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * len(filters))
    frame = scarlet.Frame(images.shape, psf=model_psf, channels=filters, dtype=dtype)
    obs = scarlet.Observation(images, psf=scarlet.ImagePSF(psfs), weights=weights,
                              channels=filters).match(frame)
    sources, _ = init_all_sources(frame, centers, obs, max_components=1, min_snr=50, thresh=1,
                                  fallback=True, silent=True, set_spectra=True)
    sources = list(sources)
    for k, spec in PROFILES.items():
        if spec[0] == "gaussian":
            sources[k] = scarlet.GaussianSource(frame, centers[k], spec[1], np.array(spec[2]), obs)
        else:
            sources[k] = scarlet.SpergelSource(frame, centers[k], spec[1], spec[2],
                                               np.array(spec[3]), obs)
    return frame, obs, sources, centers


def six(morphology):
    out = np.zeros(6)
    for name in GROUPS:
        p = morphology.get_parameter(name)
        if p is not None:
            out[SLOTS[name]] = np.array(p)
    return out


def box_table(scarlet, frame):
    from scarlet.model import UpdateException

    first, after, raised = [], [], []
    for c0, r0, c1, r1 in BOX_CASES:
        center = scarlet.Parameter(np.array(c0), name="center", step=0.01)
        radius = scarlet.Parameter(np.array((r0,)), name="radius", step=0.1)
        m = scarlet.GaussianMorphology(frame, center, radius)
        first.append(tuple(m.bbox.origin[-2:]) + (m.bbox.shape[-1],))
        center[:] = c1
        radius[:] = r1
        try:
            m.update()
            raised.append(False)
        except UpdateException:
            raised.append(True)
        after.append(tuple(m.bbox.origin[-2:]) + (m.bbox.shape[-1],))
        want = m.get_box()
        assert tuple(want.origin[-2:]) + (want.shape[-1],) == after[-1]
    return dict(box_cases=np.array([c0 + (r0,) + c1 + (r1,) for c0, r0, c1, r1 in BOX_CASES]),
                box_first=np.array(first), box_after=np.array(after), box_raised=np.array(raised))


def profile_source():
    import scipy.special

    scarlet = load_scarlet()
    import scarlet.morphology as ref_morphology

    frame, obs, sources, centers = build(scarlet, np.float32)
    blend = scarlet.Blend(sources, obs)
    model = blend.get_model()
    kinds = ["extended"] * len(sources)
    for k, spec in PROFILES.items():
        kinds[k] = spec[0]
    out = dict(model=model, rendered=obs.render(model), logL=obs.get_log_likelihood(model),
               n_sources=len(sources), kinds=np.array(kinds), fd_h=FD_H,
               sky_coords=np.array(centers, dtype=np.float64))
    out.update(box_table(scarlet, frame))
    for k, src in enumerate(sources):
        spectrum, morphology = src.children
        sed = spectrum.parameters[0]
        out["sed_%d" % k] = np.array(sed)
        out["origin_%d" % k] = np.array(morphology.bbox.origin[-2:])
        out["shape_%d" % k] = np.array(morphology.bbox.shape[-2:])
        step = sed.step
        out["sed_step_factor_%d" % k] = step.keywords.get("factor", 0.1)
        out["sed_step_minimum_%d" % k] = np.asarray(step.keywords.get("minimum", 0), dtype=np.float64)
        out["sed_zero_%d" % k] = sed.constraint.zero
        if kinds[k] == "extended":
            out["morph_%d" % k] = np.array(morphology.parameters[0])
            continue
        out["params_%d" % k] = six(morphology)
        out["morph_%d" % k] = np.array(morphology.get_model(), dtype=np.float64)
        own = morphology.parameters
        out["pnames_%d" % k] = np.array([p.name for p in own])
        out["pdtypes_%d" % k] = np.array([str(p.dtype) for p in own])
        out["pshapes_%d" % k] = np.array([p.shape[0] for p in own])
        out["pfixed_%d" % k] = np.array([bool(p.fixed) for p in own])
        out["pstep0_%d" % k] = np.array(
            [float(np.asarray(p.step(p, it=0) if callable(p.step) else p.step)) for p in own])
        out["integral_%d" % k] = np.asarray(morphology.integral, dtype=np.float64)
        assert src.center is morphology.center

    # the float64 frame: finite differences of the reference's own log-likelihood
    frame64, obs64, sources64, _ = build(scarlet, np.float64)
    blend64 = scarlet.Blend(sources64, obs64)
    owners = list(blend64.parameters)
    # (named copies: the reference's morphologies look their parameters up by name)
    params = [scarlet.Parameter(np.array(p, dtype=np.float64), name=p.name) for p in owners]

    def logL_at(at, idx, delta):
        trial = [p.copy() if i == at else p for i, p in enumerate(params)]
        trial[at][idx] += delta
        return obs64.get_log_likelihood(blend64.get_model(*trial))

    def central(at, idx, h):
        return (logL_at(at, idx, h) - logL_at(at, idx, -h)) / (2 * h)

    def index_of(p):
        return [i for i, q in enumerate(owners) if q is p][0]

    true_kv = ref_morphology.kv
    for k, src in enumerate(sources64):
        spectrum, morphology = src.children
        sed = spectrum.parameters[0]
        if not np.array_equal(np.array(sed), out["sed_%d" % k]):
            out["sed64_%d" % k] = np.array(sed)
        assert tuple(morphology.bbox.origin[-2:]) == tuple(out["origin_%d" % k])
        if kinds[k] == "extended":
            if not np.array_equal(np.array(morphology.parameters[0]), out["morph_%d" % k]):
                out["morph64_%d" % k] = np.array(morphology.parameters[0])
            continue
        assert np.array_equal(six(morphology), out["params_%d" % k])
        at = index_of(sed)
        out["fd_sed_%d" % k] = np.array([[central(at, c, h) for c in range(len(sed))]
                                         for h in (FD_H, FD_H / 2)])
        fd = np.full((2, 6), np.nan)
        for name in GROUPS:
            p = morphology.get_parameter(name)
            if p is None:
                continue
            at = index_of(p)
            if name == "nu":
                out["fd_nu_unfrozen_%d" % k] = np.array([central(at, 0, h) for h in (FD_H, FD_H / 2)])
                order = float(p[0])
                # the fit's rule: no derivative through the order of K
                ref_morphology.kv = lambda n, x, order=order: scipy.special.kv(order, x)
            try:
                for j in range(len(p)):
                    for i, h in enumerate((FD_H, FD_H / 2)):
                        fd[i, SLOTS[name].start + j] = central(at, j, h)
            finally:
                ref_morphology.kv = true_kv
        out["fd_param_%d" % k] = fd
    assert obs64.weights.dtype == np.float64
    if not np.array_equal(obs64.weights, obs.weights.astype(np.float64)):
        out["weights64"] = np.array(obs64.weights)
    out["diff_kernel64"] = np.array(obs64.renderer.diff_kernel.image)
    model64 = blend64.get_model()
    out["logL64"] = obs64.get_log_likelihood(model64)
    path = os.path.join(GOLDEN, "profile_source.npz")
    save_deterministic(path, out)
    print("profile_source.npz: %d bytes, kinds %s, logL %.3f, boxes %s"
          % (os.path.getsize(path), kinds, out["logL"],
             [tuple(out["origin_%d" % k]) + tuple(out["shape_%d" % k]) for k in PROFILES]))


if __name__ == "__main__":
    so = os.path.join(REPO, "oracle", "liboracle.so")
    had_so = os.path.exists(so)
    profile_source()
    if not had_so and os.path.exists(so):  # built in the tree by the shims on first use
        os.remove(so)
