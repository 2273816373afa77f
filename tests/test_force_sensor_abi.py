"""Force sensor tensor, the parts that need no GPU: the header declares
tg_set_force_sensor_tensor and TG_FS_MAX_SENSORS, has the index entry and fixes
the definition; tg_contact_frame is shared with tg_contact_inverse_dynamics,
not duplicated; the library exports the symbol, the ctypes binding has its
argument types, a null sim is rejected; Sim, VecTask and the walk task have
the methods and the option."""
import ctypes as C
import inspect
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tg_set_force_sensor_tensor"


def _header():
    with open(os.path.join(REPO, "include", "tgsim.h")) as f:
        return f.read()


def _flat(s):
    return " ".join(s.replace("*", " ").split())


def test_header_declares_the_entry_point_and_the_constant():
    from thormang_isaacgym_amd import abi
    text = _header()
    assert re.search(r"^int\s+%s\(tg_sim \*sim, const tg_contact_frame \*sensors" % NAME, text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int %s(" % NAME):].split(";")[0], flags=re.S))
    assert decl == _flat("int tg_set_force_sensor_tensor(tg_sim *sim, const tg_contact_frame *sensors , "
                         "int32_t num_sensors, int32_t space , float *out )")
    mx = re.search(r"^#define TG_FS_MAX_SENSORS\s+(\d+)\b", text, re.M)
    assert mx and int(mx.group(1)) == abi.TG_FS_MAX_SENSORS == 8
    for n, v in (("TG_ENV_SPACE", abi.TG_ENV_SPACE), ("TG_LOCAL_SPACE", abi.TG_LOCAL_SPACE)):
        assert int(re.search(r"^#define %s\s+(\d+)\b" % n, text, re.M).group(1)) == v


def test_contact_frame_is_shared_not_duplicated():
    from thormang_isaacgym_amd import abi
    text = _header()
    assert len(re.findall(r"typedef struct tg_contact_frame", text)) == 1
    assert len(re.findall(r"typedef struct \w*sensor\w*", text)) == 0
    # the declaration follows the struct it uses
    assert text.index("} tg_contact_frame;") < text.index("int %s(" % NAME)
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "abi.py")) as f:
        src = f.read()
    assert len(re.findall(r"^class tg_contact_frame\b", src, re.M)) == 1
    assert not re.search(r"^class \w*sensor\w*\(C\.Structure\)", src, re.M | re.I)
    assert C.sizeof(abi.tg_contact_frame) == 16


def test_header_index_has_the_entry():
    head = _flat(_header()[:_header().index("#ifndef")])
    entry = head[head.index(" %s " % NAME):head.index(" tg_jacobians ")]
    assert "acquire_force_sensor_tensor" in entry and "refresh_force_sensor_tensor" in entry
    assert "tasks/humanoid.py" in entry


def test_header_fixes_the_definition():
    text = _header()
    body = _flat(text[text.index("acquire_force_sensor_tensor (with create_asset_force_sensor implied)"):
                      text.index("#define TG_FS_MAX_SENSORS")])
    for phrase in ("p_k = o_l + R_l offset_k", "the convention of tg_contact_frame and tg_ik_chain.offset",
                   "the same link may carry several sensors", "read during the call and copied",
                   "out [N, S, 6]", "kept alive by the caller", "newtons and newton metres",
                   "GROUND REACTION on the sensor's link", "not IsaacGym's joint-transmitted constraint force",
                   "no gravity or inertial part", "nothing from the links further down the chain",
                   "Written in full by every later tg_simulate", "averaged over that call's substeps",
                   "the normal rows, the two patch-friction rows and the torsion row",
                   "stored-velocity multiplier", "f = (1 / h) sum_j lambda_j d_j",
                   "n = (1 / h) sum_j lambda_j ((x_j - p_k) x d_j + t_j)",
                   "posed from the state the substep starts from",
                   "the very sum the net contact force tensor holds", "the torsion row, which carries no force",
                   "TG_ENV_SPACE gives world axes", "TG_LOCAL_SPACE the link's own axes",
                   "(-n_y / f_z, n_x / f_z)", "A sensor on a link without collision shapes reads zeros",
                   "a simulate with 0 substeps", "zero-fills out, stream-ordered", "a reset does not clear it",
                   "refresh_force_sensor_tensor has nothing to do", "out == NULL or num_sensors == 0 turns it off",
                   "one launch for any combination", "run their post-physics as a separate launch",
                   "TG_ERR_ARG", "tg_set_force_sensor_tensor: ...", "a null sim",
                   "num_sensors outside 0..TG_FS_MAX_SENSORS", "null sensors with num_sensors > 0",
                   "a link outside [0, L)", "a non-finite offset", "space outside {0, 1}",
                   "a non-null out with num_sensors == 0", "TG_ERR_MODEL for a model from tg_model_jit",
                   "A rejected call changes nothing"):
        assert phrase in body, phrase


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_contact_frame), C.c_int32, C.c_int32, C.c_void_p]
    assert _lib.SIGNATURES[NAME] == sig
    f = getattr(_lib.lib(), NAME)
    assert f.argtypes == sig and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    frames = (abi.tg_contact_frame * 1)()
    assert f(None, frames, 1, 0, None) == -1   # TG_ERR_ARG
    assert _lib.lib().tg_last_error().startswith(b"tg_set_force_sensor_tensor: null tg_sim")


def test_sim_task_and_walk_have_the_methods_and_the_option():
    import yaml
    from thormang_isaacgym_amd.sim import Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    for cls in (Sim, VecTask):
        got = [(p.name, p.default) for p in
               list(inspect.signature(cls.acquire_force_sensor_tensor).parameters.values())[1:]]
        assert got == [("sensors", inspect.Parameter.empty), ("space", "env")], (cls, got)
        assert list(inspect.signature(cls.refresh_force_sensor_tensor).parameters) == ["self"]
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "tasks", "thormang_walk.py")) as f:
        src = f.read()
    assert 'env.get("enableFootForceSensors", False)' in src and 'extras["feet_force_sensor"]' in src
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task", "ThormangWalk.yaml")) as f:
        assert "enableFootForceSensors" not in yaml.safe_load(f)["env"]   # off by default


def test_sole_centre_is_the_bottom_face_of_the_foot_box():
    import numpy as np
    from thormang_isaacgym_amd.sim import load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_centre
    m = load_model("thormang")
    feet = walk_feet_indices(m)
    assert [m.links[l].name for l in feet] == ["l_leg_foot_link", "r_leg_foot_link"]
    for l in feet:
        s = next(s for s in m.shapes if m.link_index(s.link) == l)
        c = np.asarray(walk_sole_centre(m, l))
        rot, pos = np.asarray(s.rot, np.float64).reshape(3, 3), np.asarray(s.pos, np.float64)
        b = rot.T @ (c - pos)   # in the box's own frame: on one face, at its centre
        k = int(np.argmax(np.abs(b)))
        assert abs(abs(b[k]) - s.params[k]) < 1e-12 and np.abs(np.delete(b, k)).max() < 1e-12
        # the face looks along the link's -z: no point of the box lies lower in the link frame
        low = min((pos + rot @ (np.array([sx, sy, sz]) * np.asarray(s.params[:3])))[2]
                  for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1))
        assert abs(c[2] - low) < 1e-9
