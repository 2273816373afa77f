"""Centroidal quantities, the parts that need no GPU: the header declares
tg_centroidal and TG_CENTROIDAL_STATE, has the index entry and fixes the
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


def test_header_declares_the_entry_point_and_the_constant():
    text = _header()
    assert re.search(r"^int\s+tg_centroidal\(tg_sim \*sim,", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_centroidal("):].split(";")[0], flags=re.S))
    assert decl == _flat("int tg_centroidal(tg_sim *sim, float *state, float *matrix, float *bias)")
    assert re.search(r"^#define TG_CENTROIDAL_STATE\s+16\b", text, re.M)
    from thormang_isaacgym_amd import abi
    assert abi.TG_CENTROIDAL_STATE == 16


def test_header_index_has_the_entry():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_centroidal "):head.index("tg_get_sim_params")]
    assert "centroidal momentum matrix" in entry and "centre of mass" in entry and "h_G = A_G u" in entry


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("Centroidal quantities of the floating-base robot"):
                      text.index("#define TG_CENTROIDAL_STATE")])
    for phrase in ("stream-ordered", "body mass scales (tg_set_body_mass_scale_indexed)",
                   "nothing of the sim is written", "nothing is kept on the host between calls",
                   "a NULL output is not touched", "every element of every non-NULL output is written",
                   "exactly those of tg_jacobians and tg_mass_matrices",
                   "m'_l = s_l m_l", "I'_l = s_l R_l I_l R_l^T", "M = sum_l m'_l", "c = sum_l m'_l c_l / M",
                   "A = sum_l [ m'_l Jv_l ; I'_l Jw_l + (c_l - c) x m'_l Jv_l ]",
                   "rows 0..2 of A give the linear momentum", "rows 3..5 the angular momentum about c",
                   "A[0:3] / M is the CoM Jacobian",
                   "[0:3] c, in the world frame of tg_rigid_body_states", "[3:6] c', the CoM velocity",
                   "[6:9] k, the angular momentum about c", "[9] M",
                   "[10:16] I_G = sum_l (I'_l + m'_l (|d|^2 1 - d d^T)), d = c_l - c",
                   "xx yy zz xy xz yz of link_inertia", "A u = (M c', k)",
                   "column layout of tg_jacobians", "DOF d at column 6 + d", "Armature does not enter",
                   "A locked DOF is an ordinary column", "its dof_state velocity enters the state",
                   "A[0:3, 0:3] = M 1 with exact 0.0 off the diagonal", "A[3:6, 0:3] = 0.0",
                   "A[3:6, 3:6] = I_G", "A[0:3, 3:6] = -M [c - c_root]x",
                   "With fix_base the call still writes the full layout", "matrix[:, :, 6:] is the fixed-base view",
                   "bias[e] = A' u", "at u' = 0 without gravity", "h_G' = A u' + bias",
                   "velocity-product inertial forces", "tg_inverse_dynamics(TG_ID_VELOCITY)",
                   "relative to the root link's origin", "added last",
                   "every output other than state[0:3] is bit-identical",
                   "TG_ERR_ARG", "tg_centroidal: ...", "a null sim", "all NULL",
                   "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p] * 4
    assert _lib.SIGNATURES["tg_centroidal"] == sig
    f = _lib.lib().tg_centroidal
    assert f.argtypes == sig and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    assert f(None, None, None, None) == -1   # TG_ERR_ARG
    assert _lib.lib().tg_last_error().startswith(b"tg_centroidal: null tg_sim")


def test_python_layers_have_the_method():
    from thormang_isaacgym_amd.sim import Centroidal, Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    want = [("matrix", False), ("bias", False), ("out", None), ("out_matrix", None), ("out_bias", None)]
    for cls in (Sim, VecTask):
        assert callable(getattr(cls, "centroidal")), cls.__name__
        got = [(p.name, p.default) for p in list(inspect.signature(cls.centroidal).parameters.values())[1:]]
        assert got == want, (cls.__name__, got)
    assert Centroidal._fields == ("state", "matrix", "bias")


def test_walk_task_option_is_optional_and_off_in_the_shipped_config():
    import yaml
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "tasks", "thormang_walk.py")) as f:
        src = f.read()
    assert 'env.get("enableCentroidalState", False)' in src and 'extras["centroidal"]' in src
    cfg_dir = os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task")
    with open(os.path.join(cfg_dir, "ThormangWalk.yaml")) as f:
        assert "enableCentroidalState" not in yaml.safe_load(f)["env"]


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_centroidal" in line and "centroidal(" in line and "enableCentroidalState" in line
               and line.lstrip().startswith("|") for line in text.splitlines())
