"""Golden vectors of monotonic starlet sources: ``tests/golden/starlet_monotonic.npz``.

BUILD-CONTAINER TOOLING (the reference checkout must be present):

    python tools/make_golden_starlet_monotonic.py

Scene and import path are those of ``tools/make_golden_starlet.py``: the quickstart scene
``hsc_cosmos_35`` with ``init_all_sources(max_components=1)``, sources 0 and 2 turned into
starlet sources by ``StarletSource.from_source(src, monotonic=True)`` and the full-frame
``StarletSource(frame, monotonic=True)`` under ``np.random.seed(0)`` appended, on a float32
frame.  Recorded per starlet source: coefficients, the attributes of their
``MonotonicMaskConstraint``, step, box and spectrum; what the reference's constraint makes of the
coefficients as built and of a perturbed copy (noise of 1 % of the stack's peak, stored); and the
blend's model, rendering and logL.  The other sources are those of ``starlet_source.npz``.
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_golden_starlet import GOLDEN, REFERENCE, STARLET_OF, load_scarlet, save_deterministic  # noqa: E402

NOISE = 1e-2
SEED = 5


def build(scarlet):
    from scarlet.initialization import init_all_sources

    d = np.load(os.path.join(REFERENCE, "data", "hsc_cosmos_35.npz"))
    images, psfs = d["images"], d["psfs"]
    filters = [str(f) for f in d["filters"]]
    weights = 1 / d["variance"]
    centers = [(s["y"], s["x"]) for s in d["catalog"]]
    model_psf = scarlet.GaussianPSF(sigma=(0.8,) * len(filters))
    frame = scarlet.Frame(images.shape, psf=model_psf, channels=filters, dtype=np.float32)
    obs = scarlet.Observation(images, psf=scarlet.ImagePSF(psfs), weights=weights,
                              channels=filters).match(frame)
    sources, _ = init_all_sources(frame, centers, obs, max_components=1, min_snr=50, thresh=1,
                                  fallback=True, silent=True, set_spectra=True)
    sources = list(sources)
    for k in STARLET_OF:
        sources[k] = scarlet.StarletSource.from_source(sources[k], monotonic=True)
    np.random.seed(0)
    sources.append(scarlet.StarletSource(frame, monotonic=True))
    return frame, obs, sources


def main():
    scarlet = load_scarlet()
    frame, obs, sources = build(scarlet)
    blend = scarlet.Blend(sources, obs)
    model = blend.get_model()
    starlet = [k for k, s in enumerate(sources) if isinstance(s, scarlet.StarletSource)]
    out = dict(model=model, rendered=obs.render(model), logL=obs.get_log_likelihood(model),
               n_sources=len(sources), starlet_of=np.array(starlet), noise=NOISE)
    rng = np.random.default_rng(SEED)
    for k in starlet:
        spectrum, morphology = sources[k].children
        assert morphology.monotonic is True
        coeffs = morphology.parameters[0]
        constraint = coeffs.constraint
        values = np.array(coeffs)
        out["sed_%d" % k] = np.array(spectrum.parameters[0])
        out["origin_%d" % k] = np.array(morphology.bbox.origin[-2:])
        out["shape_%d" % k] = np.array(morphology.bbox.shape[-2:])
        out["coeffs_%d" % k] = values
        out["step_%d" % k] = coeffs.step
        out["constraint_type_%d" % k] = type(constraint).__name__
        out["center_%d" % k] = np.array(constraint.center)
        out["center_radius_%d" % k] = constraint.center_radius
        out["variance_%d" % k] = constraint.variance
        out["max_iter_%d" % k] = constraint.max_iter
        out["once_%d" % k] = constraint(values.copy(), 0)
        perturbed = values + NOISE * np.abs(values).max() * rng.standard_normal(values.shape)
        out["perturbed_%d" % k] = perturbed
        out["perturbed_once_%d" % k] = constraint(perturbed.copy(), 0)
    path = os.path.join(GOLDEN, "starlet_monotonic.npz")
    save_deterministic(path, out)
    print("starlet_monotonic.npz: %d bytes, starlet sources %s, logL %.3f"
          % (os.path.getsize(path), starlet, out["logL"]))


if __name__ == "__main__":
    so = os.path.join(REPO, "oracle", "liboracle.so")
    had_so = os.path.exists(so)
    main()
    if not had_so and os.path.exists(so):  # built in the tree by the shims on first use
        os.remove(so)
