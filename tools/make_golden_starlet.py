"""Golden vectors of the starlet source model: ``tests/golden/starlet_source.npz`` and
``tests/golden/lsbg.npz``.

BUILD-CONTAINER TOOLING (the reference checkout must be present):

    python tools/make_golden_starlet.py            # starlet_source.npz
    python tools/make_golden_starlet.py lsbg       # lsbg.npz (needs a Python that can
                                                   # unpickle the reference's data/lsbg.pkl)

The reference is imported through ``oracle.refshim.load_reference`` (pattern of
``tools/make_golden_detect.py``).  Scene: the quickstart scene ``hsc_cosmos_35`` with
``init_all_sources(max_components=1)``, sources 0 and 2 turned into starlet sources by
``StarletSource.from_source`` and the tutorial's full-frame ``StarletSource(frame)`` under
``np.random.seed(0)`` appended -- once on a float32 frame (model, rendering, logL) and once on a
float64 frame (central finite differences of the reference's own log-likelihood).
"""

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle.refshim.load_reference import REFERENCE  # noqa: E402  (only names the checkout)

GOLDEN = os.path.join(REPO, "tests", "golden")
STARLET_OF = (0, 2)
N_FD = 14
FD_H = 1e-3


def save_deterministic(path, arrays):
    """np.savez_compressed without the time stamps: the same inputs give the same bytes"""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def load_scarlet():
    """The reference under the import shims, on top of the pure-Python footprint code."""
    import detect_oracle

    sys.modules["scarlet.detect_pybind11"] = detect_oracle.as_module()
    from oracle.refshim import load_reference

    return load_reference.load()


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
    for k in STARLET_OF:
        sources[k] = scarlet.StarletSource.from_source(sources[k])
    np.random.seed(0)
    sources.append(scarlet.StarletSource(frame))
    return frame, obs, sources


def starlet_indices(scarlet, sources):
    return [k for k, s in enumerate(sources) if isinstance(s, scarlet.StarletSource)]


def starlet_source():
    scarlet = load_scarlet()
    frame, obs, sources = build(scarlet, np.float32)
    blend = scarlet.Blend(sources, obs)
    model = blend.get_model()
    out = dict(model=model, rendered=obs.render(model), logL=obs.get_log_likelihood(model),
               n_sources=len(sources), starlet_of=np.array(starlet_indices(scarlet, sources)),
               fd_h=FD_H)
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
        if not isinstance(src, scarlet.StarletSource):
            out["morph_%d" % k] = np.array(morphology.parameters[0])
            continue
        coeffs = morphology.parameters[0]
        assert coeffs.name == "coeffs" and coeffs.step == 1e-2
        values = np.array(coeffs)
        out["coeffs_%d" % k] = values
        if k in STARLET_OF:  # the image from_source transformed (the random one: seed 0)
            out["image_%d" % k] = np.array(morphology.transform.image)
        out["norm_%d" % k] = morphology.transform.norm
        chain = coeffs.constraint
        hard = chain.constraints[1].f.keywords  # partial(prox_hard, thresh=, type=)
        out["thresh_%d" % k] = np.array([t.flat[0] for t in hard["thresh"]])
        assert all(np.all(t == t.flat[0]) for t in hard["thresh"])
        out["chain_types_%d" % k] = np.array([type(c).__name__ for c in chain.constraints])
        out["l0_type_%d" % k] = hard["type"]
        once = chain(values.copy(), 0)
        out["chain_once_support_%d" % k] = np.packbits((once != 0).ravel())
        out["chain_once_sum_%d" % k] = once.sum(axis=(1, 2))

    # central finite differences of the reference's own log-likelihood, float64 frame
    frame64, obs64, sources64 = build(scarlet, np.float64)
    blend64 = scarlet.Blend(sources64, obs64)
    params = [np.array(p, dtype=np.float64) for p in blend64.parameters]
    owners = [p for p in blend64.parameters]
    rng = np.random.default_rng(11)
    for k in starlet_indices(scarlet, sources64):
        coeffs = sources64[k].children[1].parameters[0]
        at = [i for i, p in enumerate(owners) if p is coeffs][0]
        P, h, w = coeffs.shape
        picks = [(P - 1, h // 2, w // 2), (P - 1, 0, 0), (0, 0, w - 1), (1, h - 1, 0),
                 (P - 2, h - 1, w - 1), (0, h // 2, 0)]
        while len(picks) < N_FD:
            picks.append((int(rng.integers(P)), int(rng.integers(h)), int(rng.integers(w))))
        fd = []
        for idx in picks:
            vals = []
            for sign in (+1, -1):
                trial = [p.copy() if i == at else p for i, p in enumerate(params)]
                trial[at][idx] += sign * FD_H
                vals.append(obs64.get_log_likelihood(blend64.get_model(*trial)))
            fd.append((vals[0] - vals[1]) / (2 * FD_H))
        out["fd_index_%d" % k] = np.array(picks, dtype=np.int32)
        out["fd_dlogL_%d" % k] = np.array(fd)
    # the float64 build's parameters, where they differ from the float32 build's
    for k, src in enumerate(sources64):
        spectrum, morphology = src.children
        for name, value in (("sed", spectrum.parameters[0]), (
                "coeffs" if isinstance(src, scarlet.StarletSource) else "morph",
                morphology.parameters[0])):
            if not np.array_equal(np.array(value), out["%s_%d" % (name, k)]):
                out["%s64_%d" % (name, k)] = np.array(value)
        assert tuple(morphology.bbox.origin[-2:]) == tuple(out["origin_%d" % k])
    # (the observation of the float64 frame: the weights are those of the hsc_cosmos_35
    # fixture, the difference kernel is matched in float64)
    assert obs64.weights.dtype == np.float64
    if not np.array_equal(obs64.weights, obs.weights.astype(np.float64)):
        out["weights64"] = np.array(obs64.weights)
    out["diff_kernel64"] = np.array(obs64.renderer.diff_kernel.image)
    model64 = blend64.get_model()
    out["logL64"] = obs64.get_log_likelihood(model64)
    path = os.path.join(GOLDEN, "starlet_source.npz")
    save_deterministic(path, out)
    print("starlet_source.npz: %d bytes, starlet sources %s, logL %.3f"
          % (os.path.getsize(path), list(out["starlet_of"]), out["logL"]))


def lsbg():
    import pickle

    # the pickle holds an astropy WCS (dropped below): it loads where astropy is installed,
    # with the aliases NumPy has removed since put back
    for name, alias in (("asscalar", lambda a: a.item()), ("alen", len), ("float", float),
                        ("int", int), ("bool", bool), ("object", object), ("complex", complex),
                        ("str", str)):
        if name not in np.__dict__:
            setattr(np, name, alias)
    with open(os.path.join(REFERENCE, "data", "lsbg.pkl"), "rb") as f:
        data = pickle.load(f)
    out = dict(images=np.asarray(data["images"], dtype=np.float32),
               psfs=np.asarray(data["psfs"], dtype=np.float32),
               channels=np.array([str(c) for c in data["channels"]]))
    path = os.path.join(GOLDEN, "lsbg.npz")
    save_deterministic(path, out)
    print("lsbg.npz: %d bytes, images %s" % (os.path.getsize(path), out["images"].shape))


if __name__ == "__main__":
    so = os.path.join(REPO, "oracle", "liboracle.so")
    had_so = os.path.exists(so)
    if "lsbg" in sys.argv[1:]:
        lsbg()
    else:
        starlet_source()
    if not had_so and os.path.exists(so):  # built in the tree by the shims on first use
        os.remove(so)
