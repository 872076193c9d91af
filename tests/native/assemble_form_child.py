"""Child of tests/test_gpu_assemble.py::test_both_forms_are_byte_identical_to_upload: each form of the
gather (TT_ASSEMBLE_FORM) runs in a process of its own here. Assembles scene S from one object per BLAS and prints
sha1 digests of the scene's nodes and triangles read back, and of a frame's records traced on it."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "truetrace-unity-pathtracer_amd", "python"))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import assemble_cases as AC  # noqa: E402
import tthip  # noqa: E402

W = H = 64
am, s = AC.scene_s()
eng = tthip.Engine(0)
_, objects = am.assemble(eng)
nodes, tris = eng.scene_nodes(0, len(s.nodes)), eng.scene_tris(0, len(s.tris))
c2w, ip = tthip.unity_camera((0, 2, 14), (0, -0.1, -1), (0, 1, 0), 55, W, H, 0.3, 1000.0)
rays = np.zeros(2 * W * H, tthip.RAY_DTYPE)
eng.generate(rays, c2w, ip, W, H, 0.3, 1000.0, jitter=1, frames=3, max_bounce=1)
info = np.zeros((W * H, 4), np.uint32)
eng.trace(rays, W * H, 0, 1000.0, W, H, info=info)
for o in objects:
    o.destroy()
eng.close()
print("RESULT", os.environ.get("TT_ASSEMBLE_FORM", ""), hashlib.sha1(nodes.tobytes()).hexdigest(),
      hashlib.sha1(tris.tobytes()).hexdigest(), hashlib.sha1(rays.tobytes() + info.tobytes()).hexdigest())
