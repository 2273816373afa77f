"""Operational-space control, the parts that need no GPU: the header declares
tg_osc and tg_osc_gains, lists the reference counterpart and fixes the
definitions; the library exports the symbol, the ctypes binding has its
argument types and the structure's size, a null sim is rejected; the Python
layers have the method and INTEGRATION.md has the row."""
import ctypes as C
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "tgsim.h")) as f:
        return f.read()


def _flat(s):
    return " ".join(s.replace("*", " ").split())


def test_header_declares_the_entry_point_and_the_gains():
    text = _header()
    assert re.search(r"^int\s+tg_osc\(tg_sim \*sim, const tg_ik_chain \*chains /\* HOST \*/, int32_t num_chains,",
                     text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_osc("):].split(";")[0], flags=re.S))
    assert decl == _flat("int tg_osc(tg_sim *sim, const tg_ik_chain *chains , int32_t num_chains, "
                         "const float *goal_pos, const float *goal_quat, const float *q_rest, "
                         "const tg_osc_gains *gains, float *tau, float *err, float *efforts)")
    struct = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct tg_osc_gains"):text.index("} tg_osc_gains;")],
                          flags=re.S))
    assert struct == _flat("typedef struct tg_osc_gains { float kp, kd; float kp_null, kd_null; float damping;")


def test_header_lists_the_reference_counterpart():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_osc "):head.index("tg_get_sim_params")]
    assert "tasks/franka_cube_stack.py:602-628" in entry and "_compute_osc_torques" in entry


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("Operational-space control, _compute_osc_torques"):
                      text.index("typedef struct tg_osc_gains")])
    for phrase in ("tau = J^T Lambda (kp err - kd v) + (H_c a - J^T Lambda (J a))",
                   "Lambda = (J H_c^-1 J^T + lambda^2 I)^-1",
                   "x = o_l + R_l offset on the link ORIGIN", "the base is held fixed", "exactly-0 column",
                   "locked DOF is an ordinary column", "q_goal is normalised by the kernel",
                   "err[3:6] is written as 0 without goal_quat",
                   "H_c (nd x nd) = H[6 + dofs[i], 6 + dofs[j]] with H as tg_mass_matrices defines it",
                   "body mass scale and its TG_PROP_ARMATURE row included", "the reference's mm[:, :7, :7]",
                   "v = J qd_c", "with the base held", "equals the reference's eef_vel",
                   "both inverses by Cholesky",
                   "a = kp_null w(q_rest - q) - kd_null qd",
                   "w(x) = x - 2 pi floor((x + pi) / (2 pi)) for a revolute DOF",
                   "w(x) = x for a prismatic one", "tau += H_c a - J^T Lambda (J a)",
                   "(I - J^T Jbar) H a with Jbar = Lambda J H_c^-1",
                   "exactly 0.0 for the padding c >= num_dofs", "every element of tau and err is written",
                   "Without q_rest an off-path column's tau is exactly 0.0", "tau is not clamped",
                   "in ascending (k, c) order, no atomics", "-TG_PROP_EFFORT[e, d], +TG_PROP_EFFORT[e, d]",
                   "No other element of efforts is touched", "dof_actuation",
                   "nothing of the sim is written", "HOST memory, read during the call and not retained",
                   "TG_ERR_ARG", "tg_osc:", "null gains", "tau, err and efforts all NULL",
                   "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def test_gains_structure_layout():
    from thormang_isaacgym_amd import abi
    assert C.sizeof(abi.tg_osc_gains) == 20
    assert [f[0] for f in abi.tg_osc_gains._fields_] == ["kp", "kd", "kp_null", "kd_null", "damping"]
    assert [getattr(abi.tg_osc_gains, f).offset for f in ("kp", "kd", "kp_null", "kd_null", "damping")] == \
        [0, 4, 8, 12, 16]


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_ik_chain), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
           C.POINTER(abi.tg_osc_gains), C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["tg_osc"] == sig
    f = _lib.lib().tg_osc
    assert f.argtypes == sig and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    ch = (abi.tg_ik_chain * 1)()
    g = abi.tg_osc_gains(150.0, 24.5, 10.0, 6.3, 0.01)
    assert f(None, ch, 1, None, None, None, C.byref(g), None, None, None) == -1   # TG_ERR_ARG
    assert b"null tg_sim" in _lib.lib().tg_last_error()


def test_python_layers_have_the_method():
    from thormang_isaacgym_amd.sim import Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    want = [("chains", inspect.Parameter.empty), ("goal_pos", inspect.Parameter.empty), ("goal_quat", None),
            ("kp", 150.0), ("kd", None), ("kp_null", 10.0), ("kd_null", None), ("q_rest", None), ("damping", 1e-2),
            ("efforts", None), ("return_error", False)]
    for cls in (Sim, VecTask):
        assert callable(getattr(cls, "solve_osc")), cls.__name__
        got = [(p.name, p.default) for p in list(inspect.signature(cls.solve_osc).parameters.values())[1:]]
        assert got == want, (cls.__name__, got)


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_osc" in line and "tasks/franka_cube_stack.py:602-628" in line and "solve_osc" in line
               and line.lstrip().startswith("|") for line in text.splitlines())
