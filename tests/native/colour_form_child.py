"""Child of tests/test_gpu_colour.py::test_terrain_persistent_form: the terrain kernel form is chosen once per process
(TT_TERRAIN_FORM), so the other form runs here. Prints the float64 colour pin's report line for both terrain cases
and every flag combination; exits non-zero on a failure."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "truetrace-unity-pathtracer_amd", "python"))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import colour as CM  # noqa: E402
import colour_cases as CC  # noqa: E402
import terrain_cases as TC  # noqa: E402
import tthip  # noqa: E402

eng = tthip.Engine(0)
eng.upload(TC.scene())
eng.upload_terrains(TC.terrains(), TC.atlas())
bad = 0
for case in (CC.terrain_set(), CC.edge_table(CM.TERRAIN)):
    for flags in CC.FLAGS:
        for bounce in (0, 1):
            rays, col, cache = case.rays.copy(), case.col.copy(), case.cache.copy()
            vis = np.full((len(rays), 4), -7.5, np.float32)
            eng.shadow_heightmap(rays, len(rays), bounce, case.W, case.H, visibility=vis, colors=col, cache=cache,
                                 flags=flags)
            rep = CC.check(case, vis, col, cache, bounce, flags)
            bad += len(rep.fails)
            print(f"REPORT {case.name} bounce {bounce} flags {flags:#x}: {rep.text}")
            for f in rep.fails:
                print("FAIL", f)
eng.close()
sys.exit(1 if bad else 0)
