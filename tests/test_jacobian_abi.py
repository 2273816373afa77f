"""Jacobian and mass-matrix tensors, the parts that need no GPU: the header
declares tg_jacobians / tg_mass_matrices, lists their reference counterparts
and fixes the definitions; the library exports both, the ctypes binding has
their argument types, a null sim is rejected; and the Python layers pass the
tensors through."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tg_jacobians", "tg_mass_matrices")


def _header():
    with open(os.path.join(REPO, "include", "tgsim.h")) as f:
        return f.read()


def _flat(s):
    return " ".join(s.replace("*", " ").split())


@pytest.mark.parametrize("name", NAMES)
def test_header_declares_the_entry_point(name):
    assert re.search(r"^int\s+%s\(tg_sim \*sim, float \*out\);" % name, _header(), re.M)


def test_header_lists_the_reference_counterparts():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    assert "tg_jacobians" in head and "acquire_jacobian_tensor / refresh_jacobian_tensors" in head
    assert "tasks/gogoro/gogoro.py:108-114,396-397,507" in head
    assert "tg_mass_matrices" in head and "acquire_mass_matrix_tensor / refresh_mass_matrix_tensors" in head
    assert "tasks/franka_cube_stack.py:393,441" in head
    assert "tasks/franka_cube_stack.py:389-393, 440-441" in head


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("refresh_jacobian_tensors on the tensor"):text.index("int tg_jacobians(")])
    assert "out [N, L, 6, 6+D]" in body
    assert "u(0:6) exactly root_state[7:13]" in body
    assert "column 6+d is DOF d" in body
    assert "J[e, l] u == rigid_body_state[e, l, 7:13]" in body
    assert "exactly 0.0" in body and "exactly the identity" in body
    assert "locked DOF" in body and "dof_state position" in body
    assert "relative to the root link's origin" in body
    body = _flat(text[text.index("refresh_mass_matrix_tensors on the tensor"):text.index("int tg_mass_matrices(")])
    assert "out [N, 6+D, 6+D]" in body
    assert "H = sum_l s_l (m_l Jv_l^T Jv_l + Jw_l^T R_l I_l R_l^T Jw_l) + diag(0_6, armature)" in body
    assert "tg_set_body_mass_scale_indexed" in body and "TG_PROP_ARMATURE" in body
    assert "locked rows and columns removed" in body
    assert "symmetric bit for bit" in body


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_and_binds_the_symbol(name):
    from thormang_isaacgym_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    assert _lib.SIGNATURES[name] == [C.c_void_p, C.c_void_p]
    f = getattr(_lib.lib(), name)
    assert f.argtypes == [C.c_void_p, C.c_void_p] and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    assert f(None, None) == -1   # TG_ERR_ARG
    assert b"null tg_sim" in _lib.lib().tg_last_error()


def test_python_layers_pass_the_tensors_through():
    from thormang_isaacgym_amd.sim import Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    for cls in (Sim, VecTask):
        for meth in ("acquire_jacobian_tensor", "refresh_jacobian_tensors", "acquire_mass_matrix_tensor",
                     "refresh_mass_matrix_tensors"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)


def test_integration_table_has_a_row_for_each_tensor():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    for name, call in (("tg_jacobians", "acquire_jacobian_tensor"), ("tg_mass_matrices", "acquire_mass_matrix_tensor")):
        assert any(name in line and call in line and line.lstrip().startswith("|") for line in text.splitlines()), name
