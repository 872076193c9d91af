"""The differential corpus of the host scene checks (csrc/tt_scene_check_host.h): valid scenes and BLASes with one
field changed at a time, so that every refusal of the CWBVH walk and every index it computes is met from both
sides of its bound. Seeded with a generator of its own (no library's random stream), so a case's number names the
same input everywhere. Test infrastructure, no test lives here.

As a program it records what a library answers, as the file tests/test_scene_check_host.py compares with:

    TT_HIP_LIB=<a build of the commit to record>/lib/libtruetrace_hip.so python tests/scene_check_cases.py OUT.json
"""
import dataclasses
import functools
import json
import os
import sys

import numpy as np

if __name__ == "__main__":
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_here, os.path.join(os.path.dirname(_here), "truetrace-unity-pathtracer_amd", "python")]

import assemble_cases as AC
import kat_cases
import tthip

SEED = 0x5CE7E
# x 5 kinds = 200 mutations per scene, x 3 kinds = 120 per BLAS (at 30 the rarest refusal of the scene walk, the
# leaf-meta spill, came up 4 times: fewer than the 5 the test asks of every kind)
PER_KIND = 40
SCENE_KINDS = ("meta", "base_child", "base_tri", "NodeOffset", "tlas")
OBJECT_KINDS = SCENE_KINDS[:3]


class Rng:
    """splitmix64"""

    def __init__(self, seed: int):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        return z ^ (z >> 31)

    def below(self, n: int) -> int:
        return self.next() % n

    def between(self, lo: int, hi: int) -> int:
        """In [lo, hi)."""
        return lo + self.below(hi - lo)


@functools.lru_cache(maxsize=None)
def base_scenes():
    """[(name, Scene)]: a builder scene with inner nodes at both levels of the walk's arithmetic, and the first six
    hand-built known-answer scenes (one to three nodes each: every mutation lands near the root)."""
    out = [("soup200", tthip.single_object_scene(tthip.Mesh.soup(3, 200, 1.0, 0.1)))]
    for case in kat_cases.ALL_CASES[:6]:
        name, sc = case()[:2]
        out.append((name, sc))
    return out


def _mutate_nodes(rng: Rng, kind: str, nodes: np.ndarray, n_tris: int) -> np.ndarray:
    a = nodes.copy()
    ni = rng.below(len(a))
    if kind == "meta":
        a.view(np.uint8).reshape(len(a), 80)[ni, 24 + rng.below(8)] = rng.below(256)
    elif kind == "base_child":
        a["base_child"][ni] = rng.below(2 * len(a))
    else:
        a["base_tri"][ni] = rng.below(2 * n_tris)
    return a


@functools.lru_cache(maxsize=None)
def scene_cases():
    """[(label, Scene)]: PER_KIND mutations of each kind per base scene."""
    rng = Rng(SEED)
    out = []
    for name, s in base_scenes():
        for kind in SCENE_KINDS:
            for i in range(PER_KIND):
                if kind in OBJECT_KINDS:
                    m = dataclasses.replace(s, nodes=_mutate_nodes(rng, kind, s.nodes, len(s.tris)))
                elif kind == "NodeOffset":
                    md = s.meshdata.copy()
                    md["NodeOffset"][rng.below(len(md))] = rng.between(-1, 2 * len(s.nodes))
                    m = dataclasses.replace(s, meshdata=md)
                else:
                    tl = s.tlas.copy()
                    tl[rng.below(len(tl))] = rng.between(-1, len(s.meshdata) + 1)
                    m = dataclasses.replace(s, tlas=tl)
                out.append((f"{name}/{kind}/{i}", m))
    return out


@functools.lru_cache(maxsize=None)
def object_cases():
    """[(label, nodes, tris)]: PER_KIND mutations of the first three kinds per BLAS of assemble_cases (root 0)."""
    rng = Rng(SEED + 1)
    out = []
    for b, blas in enumerate(AC.meshes_and_blases()[1]):
        nodes, tris = blas.arrays()
        for kind in OBJECT_KINDS:
            for i in range(PER_KIND):
                out.append((f"blas{b}/{kind}/{i}", _mutate_nodes(rng, kind, nodes, len(tris)), tris))
    return out


def answers():
    """{"scene": [[label, status, message]], "object": [...]} of the loaded library (tthip.hip_lib)."""
    return {"scene": [[label, *tthip.validate(s)] for label, s in scene_cases()],
            "object": [[label, *tthip.object_validate(n, t)] for label, n, t in object_cases()]}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(answers(), f, indent=0)
        f.write("\n")
