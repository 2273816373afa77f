"""Damped-least-squares IK, the parts that need no GPU: the header declares
tg_ik_dls and tg_ik_chain, lists the reference counterpart and fixes the
definitions; the library exports the symbol, the ctypes binding has its
argument types and the structure's size, a null sim is rejected; and the
Python layers have the methods."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "tgsim.h")) as f:
        return f.read()


def _flat(s):
    return " ".join(s.replace("*", " ").split())


def test_header_declares_the_entry_point_and_the_chain():
    text = _header()
    assert re.search(r"^int\s+tg_ik_dls\(tg_sim \*sim, const tg_ik_chain \*chains /\* HOST \*/, int32_t num_chains,",
                     text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_ik_dls("):].split(";")[0], flags=re.S))
    assert decl == _flat("int tg_ik_dls(tg_sim *sim, const tg_ik_chain *chains , int32_t num_chains, "
                         "const float *goal_pos, const float *goal_quat, float damping, float *dq, float *err, "
                         "float *pos_targets)")
    assert re.search(r"#define TG_IK_MAX_CHAINS 8\b", text) and re.search(r"#define TG_IK_MAX_DOFS\s+8\b", text)
    struct = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct tg_ik_chain"):text.index("} tg_ik_chain;")],
                          flags=re.S))
    assert struct == _flat("typedef struct tg_ik_chain { int32_t link; int32_t num_dofs; "
                           "int32_t dofs[TG_IK_MAX_DOFS]; float offset[3];")


def test_header_lists_the_reference_counterpart():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    assert "tg_ik_dls" in head
    assert "tasks/gogoro/gogoro.py:381-427" in head
    assert re.search(r"tasks/franka_cube_stack\.py:\d+", head[head.index("tg_ik_dls"):head.index("tg_get_sim_params")])


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("Damped-least-squares end-effector IK"):text.index("#define TG_IK_MAX_CHAINS")])
    assert "x = o_l + R_l offset" in body and "link ORIGIN" in body
    assert "not the centre of mass the linear rows of tg_jacobians use" in body
    assert "a revolute column is a_j x (x - p_j), a prismatic one a_j" in body
    assert "the base is held fixed" in body
    assert "exactly-0 column" in body and "dq is exactly 0.0" in body
    assert "locked DOF is an ordinary column at its dof_state position" in body
    assert "err[0:3] = (goal_pos - root_pos) - (x - root_pos)" in body
    assert "err[3:6] = vec(q_goal (x) conj(q_l)) s, s = +1 if the product's w >= 0 and -1 otherwise" in body
    assert "q_goal normalised by the kernel" in body
    assert "err[3:6] is written as 0" in body
    assert "y = (J J^T + lambda^2 I)^-1 err by Cholesky" in body
    assert "exactly 0.0 for the padding" in body and "every element of dq and err is written" in body
    assert "pos_targets[e, d] = q[e, d] + sum of dq[e, k, c]" in body and "no atomics" in body
    assert "No other element of pos_targets is touched" in body
    assert "not clamped to the joint limits" in body
    assert "HOST memory, read during the call and not retained" in body
    assert "TG_ERR_ARG" in body and "tg_ik_dls:" in body


def test_chain_structure_layout():
    from thormang_isaacgym_amd import abi
    assert C.sizeof(abi.tg_ik_chain) == 52
    assert abi.tg_ik_chain.dofs.offset == 8 and abi.tg_ik_chain.offset.offset == 40
    assert (abi.TG_IK_MAX_CHAINS, abi.TG_IK_MAX_DOFS) == (8, 8)


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_ik_chain), C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
           C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["tg_ik_dls"] == sig
    f = _lib.lib().tg_ik_dls
    assert f.argtypes == sig and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    ch = (abi.tg_ik_chain * 1)()
    assert f(None, ch, 1, None, None, 0.3, None, None, None) == -1   # TG_ERR_ARG
    assert b"null tg_sim" in _lib.lib().tg_last_error()


def test_python_layers_have_the_methods():
    from thormang_isaacgym_amd.sim import Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    for cls in (Sim, VecTask):
        for meth in ("ik_chain", "solve_ik"):
            assert callable(getattr(cls, meth)), (cls.__name__, meth)


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_ik_dls" in line and "tasks/gogoro/gogoro.py:381-427" in line and line.lstrip().startswith("|")
               for line in text.splitlines())
