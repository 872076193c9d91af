"""Child of tests/test_gpu_terrain.py::test_persistent_form_matches: the kernel form is chosen once per process
(TT_TERRAIN_FORM), so the other form runs here. Prints sha1 digests of the GPU's bounce-1 records + info texels
and of the shadow visibility records of the randomized sets."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "truetrace-unity-pathtracer_amd", "python"))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import oracle_ctypes as O  # noqa: E402
import terrain_cases as TC  # noqa: E402
import tthip  # noqa: E402

n, off = TC.N_RANDOM, TC.RW * TC.RH
rays = np.zeros(2 * off, tthip.RAY_DTYPE)
rays[off:off + n] = TC.random_rays()
info = np.full((off, 4), 0x51515151, np.uint32)
colors = np.zeros(off, tthip.COL_DTYPE)
colors["Data"][:, 3] = -1.0
assert O.trace(TC.scene(), rays, n, 1, TC.FAR, TC.RW, TC.RH, info=info, colors=colors)[0] == 0
eng = tthip.Engine(0)
eng.upload_terrains(TC.terrains(), TC.atlas())
s = eng.trace_heightmap(rays, n, 1, TC.FAR, TC.RW, TC.RH, info=info, stats=True)
vis = np.full((TC.N_SHADOW, 4), -7.5, np.float32)
eng.shadow_heightmap(TC.shadow_rays().copy(), TC.N_SHADOW, 0, TC.SW, TC.SH, visibility=vis)
eng.close()
print("RESULT", hashlib.sha1(rays.tobytes() + info.tobytes()).hexdigest(), hashlib.sha1(vis.tobytes()).hexdigest(),
      s.hits, s.node_visits, s.reps_exhausted)
