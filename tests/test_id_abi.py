"""Inverse dynamics, the parts that need no GPU: the header declares
tg_inverse_dynamics and the TG_ID_* terms, has the index entry and fixes the
definitions; the library exports the symbol, the ctypes binding has its
argument types, a null sim is rejected; the Python layers have the method and
INTEGRATION.md has the row."""
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


def test_header_declares_the_entry_point_and_the_terms():
    text = _header()
    assert re.search(r"^int\s+tg_inverse_dynamics\(tg_sim \*sim, int32_t terms,", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_inverse_dynamics("):].split(";")[0], flags=re.S))
    assert decl == _flat("int tg_inverse_dynamics(tg_sim *sim, int32_t terms, const float *accel, float *tau, "
                         "float *efforts, const int32_t *dofs , int32_t num_dofs, int32_t accumulate)")
    assert re.search(r"^#define TG_ID_GRAVITY\s+1\b", text, re.M)
    assert re.search(r"^#define TG_ID_VELOCITY\s+2\b", text, re.M)
    from thormang_isaacgym_amd import abi
    assert (abi.TG_ID_GRAVITY, abi.TG_ID_VELOCITY) == (1, 2)


def test_header_index_has_the_entry():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_inverse_dynamics "):head.index("tg_get_sim_params")]
    assert "gravity and Coriolis compensation" in entry and "tau = H a + h" in entry


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("Inverse dynamics by one recursive Newton-Euler pass"):
                      text.index("#define TG_ID_GRAVITY")])
    for phrase in ("tau = H a + h(q, u)", "H u' + h = tau",
                   "exactly the coordinates of tg_jacobians and tg_mass_matrices",
                   "stream-ordered", "the sim's current gravity (tg_set_gravity included)",
                   "body mass scales", "TG_PROP_ARMATURE and TG_PROP_EFFORT rows", "nothing of the sim is written",
                   "HOST memory, read during the call and not retained", "bitmask",
                   "u(0:6) = root_state[7:13]", "root link's centre of mass",
                   "tau = H a + sum_l s_l [ Jv_l^T m_l (ab_l - [GRAVITY] g)",
                   "Jw_l^T (R_l I_l R_l^T alb_l + w_l x (R_l I_l R_l^T w_l))",
                   "velocity-product accelerations", "with u' held at 0", "w_l = Jw_l u",
                   "Without TG_ID_VELOCITY u is taken as 0", "H a includes the armature on the diagonal",
                   "tau[0:3] is the net force", "tau[3:6] the net moment about the root link's centre of mass",
                   "tau[6 + d] DOF d's generalised force", "Locked DOFs are ordinary entries",
                   "relative to the root link's origin", "Every element of tau is written",
                   "With fix_base the call still writes the full layout", "the reaction at the base",
                   "efforts[e, d] = clamp(t, -TG_PROP_EFFORT[e, d], +TG_PROP_EFFORT[e, d])",
                   "efforts[e, d] = clamp(efforts[e, d] + t, -TG_PROP_EFFORT[e, d], +TG_PROP_EFFORT[e, d])",
                   "No other element of efforts is touched", "dof_actuation", "this clamps twice",
                   "TG_ERR_ARG", "tg_inverse_dynamics: ...", "a null sim", "terms outside 0..3",
                   "terms == 0 with accel NULL", "tau and efforts both NULL", "num_dofs outside 0..D",
                   "dofs NULL with num_dofs > 0", "a DOF outside [0, D)", "DOF listed twice",
                   "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_int32]
    assert _lib.SIGNATURES["tg_inverse_dynamics"] == sig
    f = _lib.lib().tg_inverse_dynamics
    assert f.argtypes == sig and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    assert f(None, 3, None, None, None, None, 0, 0) == -1   # TG_ERR_ARG
    assert _lib.lib().tg_last_error().startswith(b"tg_inverse_dynamics: null tg_sim")


def test_python_layers_have_the_method():
    from thormang_isaacgym_amd.sim import Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    want = [("accel", None), ("gravity", True), ("velocity", True), ("dofs", None), ("efforts", None),
            ("accumulate", False), ("out", None)]
    for cls in (Sim, VecTask):
        assert callable(getattr(cls, "inverse_dynamics")), cls.__name__
        got = [(p.name, p.default) for p in list(inspect.signature(cls.inverse_dynamics).parameters.values())[1:]]
        assert got == want, (cls.__name__, got)


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_inverse_dynamics" in line and "inverse_dynamics(" in line and "accumulate" in line
               and line.lstrip().startswith("|") for line in text.splitlines())
