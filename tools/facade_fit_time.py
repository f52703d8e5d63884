"""Development aid: wall time of ``Blend.fit(100, e_rel=1e-4)`` for the quickstart blend
(tests/golden/hsc_cosmos_35), box resizing off and on, after a short warm-up fit.

    python tools/facade_fit_time.py
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import golden  # noqa: E402
from test_gpu_facade import build_blend  # noqa: E402

hsc = golden("hsc_cosmos_35")
blend, obs = build_blend(hsc, resizing=False)
blend.fit(5)
for r in (False, True):
    blend, obs = build_blend(hsc, resizing=r)
    t0 = time.perf_counter()
    n, logL = blend.fit(100, e_rel=1e-4)
    dt = time.perf_counter() - t0
    print("resizing", r, "iterations", n, "time %.1f ms" % (dt * 1e3))
