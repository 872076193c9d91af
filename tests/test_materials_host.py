"""The oracle against texture space: its Cutout alpha test and its stained-glass tints must be those of
materials.py, a float64 model written from the reference's text that reads neither the oracle nor the
kernels. The parity tests prove kernel == oracle bit for bit; this file pins the oracle's material path (AlignUV,
the two samplers, BaseUv from the record, the per-material rectangles and cutoffs, the tint and its conditions)
against the model, on the scenes, atlases, ray sets, caps, coverage floors and controls of materials_cases.py.
test_gpu_materials.py makes the same comparison for the kernels.

A ray whose answer could turn on a float32 rounding, in geometry or in texture space, is unrobust and only
counted; every other ray must agree exactly on miss / (mesh, triangle) or on occluded / visible, a visible
ray's visibility row must be a product of the tints it must and may cross within the bound of
materials.tint_check, and on the affine-UV scenes the UV a record gives must be the UV of that point of the mesh."""
import pytest

import bruteforce_cases as C
import materials_cases as MC
import oracle_ctypes as O
import tthip

FAR = MC.FAR
THREADS = 4


class OracleSide(MC.Side):
    def trace(self, sc, rays, n, flags, bounce):
        r = rays.copy()
        st, _ = O.trace(sc, r, n, bounce, FAR, n, 1, flags=flags, nthreads=THREADS)
        assert st == 0
        return r["hits"][n * bounce:n * bounce + n]

    def nee_frame(self, sc, c2w, ip):
        frame = O.generate(c2w, ip, C.NEE_W, C.NEE_H, 0.05, FAR)
        assert O.trace(sc, frame, C.NEE_W * C.NEE_H, 0, FAR, C.NEE_W, C.NEE_H, nthreads=THREADS)[0] == 0
        return frame

    def shadow(self, sc, before, W, H, bounce, visibility_check):
        after = before.copy()
        vis, col, nee = C.shadow_outputs(len(before), W * H)
        st, cnt = O.shadow(sc, after, len(after), bounce, W, H, visibility=vis, colors=col, nee_pos=nee, counts=True,
                           nthreads=THREADS, flags=tthip.TT_SHADOW_VISIBILITY_CHECK if visibility_check else 0)
        assert st == 0
        return after, vis, col, nee, cnt["status"]


SIDE = OracleSide()


# ------------------------------------------------------------------ closest hit, the linear sampler
@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("flags", C.FLAGS)
@pytest.mark.parametrize("ray_set", ["random", "axis"])
@pytest.mark.parametrize("name", MC.SCENES)
def test_closest_matrix(name, ray_set, flags, bounce):
    MC.closest_case(SIDE, name, "noise", ray_set, flags, bounce).check()


@pytest.mark.parametrize("flags,bounce", [(0, 1), (C.FLAGS[3], 0)])
@pytest.mark.parametrize("atlas", MC.ATLASES[1:])
@pytest.mark.parametrize("name", MC.SCENES)
def test_closest_other_atlases(name, atlas, flags, bounce):
    MC.closest_case(SIDE, name, atlas, "random", flags, bounce).check()


@pytest.mark.parametrize("name", MC.SCENES)
def test_closest_4096_rays(name):
    MC.closest_case(SIDE, name, "noise", "big", 0, 1).check()


@pytest.mark.parametrize("name", MC.AFFINE)
def test_record_uv_is_the_surface_uv(name):
    """The host builder's UV packing."""
    MC.uv_case(SIDE, name)


# ------------------------------------------------------------------ any-hit, the point sampler and the tints
@pytest.mark.parametrize("visibility_check", [False, True], ids=["default", "vischeck"])
@pytest.mark.parametrize("bounce", [0, 1])
@pytest.mark.parametrize("name,ray_set", MC.SHADOW_CASES)
def test_any_hit_matrix(name, ray_set, bounce, visibility_check):
    MC.any_hit_case(SIDE, name, "noise", ray_set, bounce, visibility_check).check()


@pytest.mark.parametrize("atlas", MC.ATLASES[1:])
@pytest.mark.parametrize("name", MC.SCENES)
def test_any_hit_other_atlases(name, atlas):
    MC.any_hit_case(SIDE, name, atlas, "random", 0, False).check()


@pytest.mark.parametrize("name", MC.SCENES)
def test_any_hit_4096_rays(name):
    MC.any_hit_case(SIDE, name, "noise", "big", 0, False).check()


@pytest.mark.parametrize("family", list(MC.FAMILIES))
def test_coverage(family):
    MC.coverage_case(SIDE, family)


# ------------------------------------------------------------------ controls: the comparison must be able to fail
@pytest.mark.parametrize("variant", MC.TEXTURE_CONTROLS)
def test_control_texture_space(variant):
    MC.control_texture_space(SIDE, variant)


def test_control_tints():
    MC.control_tints(SIDE)


def test_control_le_for_lt_at_exact_equality():
    MC.control_equality(SIDE)


def test_numpy_edits_of_a_correct_output_are_reported():
    MC.control_numpy_edits(SIDE)
