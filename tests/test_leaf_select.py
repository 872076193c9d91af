"""The selection predicate of the leaf-TLAS kernels (root_one_instance over root_leaf_of, csrc/tt_device.h)
through the C ABI (tt_tlas_root_form; host only, no device): node 0 qualifies only when it has no internal
child and exactly one child slot, a leaf, holding exactly one instance."""
import ctypes as C

import numpy as np
import pytest

import handbuilt as hb
import tthip

BOX = ((10, 20, 30), (200, 210, 220))


def _node(children):
    return np.array([hb.make_node((-8.0, -8.0, -8.0), (124, 124, 124), 3, 0, children)], tthip.NODE_DTYPE)


@pytest.mark.parametrize("slot", [0, 3, 4, 7])
@pytest.mark.parametrize("first", [0, 5])
def test_one_leaf_one_instance_qualifies(slot, first):
    assert tthip.tlas_root_form(_node([(slot, "leaf", *BOX, (first, 1))])) == tthip.TT_ROOT_ONE_INSTANCE


@pytest.mark.parametrize("count", [2, 3])
def test_one_leaf_of_several_instances_stays_generic(count):
    assert tthip.tlas_root_form(_node([(2, "leaf", *BOX, (0, count))])) == tthip.TT_ROOT_ONE_LEAF


def test_internal_child_does_not_qualify():
    assert tthip.tlas_root_form(_node([(0, "inner", *BOX, 0)])) == tthip.TT_ROOT_GENERIC
    assert tthip.tlas_root_form(_node([(0, "inner", *BOX, 0), (1, "leaf", *BOX, (0, 1))])) == tthip.TT_ROOT_GENERIC


def test_two_children_do_not_qualify():
    two = [(0, "leaf", *BOX, (0, 1)), (5, "leaf", *BOX, (1, 1))]
    assert tthip.tlas_root_form(_node(two)) == tthip.TT_ROOT_GENERIC


def test_empty_node_and_null_arguments():
    assert tthip.tlas_root_form(_node([])) == tthip.TT_ROOT_GENERIC
    L = tthip.hip_lib()
    f = C.c_uint32()
    assert L.tt_tlas_root_form(None, C.byref(f)) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_tlas_root_form(_node([]).ctypes.data, None) == tthip.TT_ERR_INVALID_ARG
    assert L.tt_trace_last_form(None, C.byref(f)) == tthip.TT_ERR_INVALID_ARG


def test_builder_scenes():
    """What the builder makes: one imported mesh is the one-instance form; the hand-built two-instance leaf is not."""
    import kat_cases as K

    assert tthip.tlas_root_form(tthip.single_object_scene(tthip.Mesh.cornell()).nodes[:1]) == tthip.TT_ROOT_ONE_INSTANCE
    assert tthip.tlas_root_form(K.case_two_instances()[1].nodes[:1]) == tthip.TT_ROOT_ONE_LEAF
