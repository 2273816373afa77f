"""The IMU, the parts that need no GPU: the header declares tg_imu, tg_imu_params
and the TG_IMU_* constants, has the index entry and fixes the definitions;
abi.py agrees with the header; the library exports the symbol and the ctypes
binding has its argument types; every argument error that can be judged without
a sim is raised -- the call checks its arguments before it looks at the sim, so
a null sim with one bad argument reports the argument, and a null sim with good
arguments reports the sim: nothing can have been launched -- the Python layers
have the methods, the task option is optional and off in the shipped config,
and INTEGRATION.md has the row.  (A link >= L needs a sim:
tests/test_gpu_imu.py.)"""
import ctypes as C
import inspect
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "tgsim.h")) as f:
        return f.read()


def _flat(s):
    return " ".join(s.replace("*", " ").split())


def test_header_declares_the_entry_point_the_struct_and_the_constants():
    text = _header()
    assert re.search(r"^int\s+tg_imu\(tg_sim \*sim,", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_imu("):].split(";")[0], flags=re.S))
    decl = re.sub(r"\s+([,)])", r"\1", decl)           # (a comment may stand between a name and its comma)
    assert decl == _flat("int tg_imu(tg_sim *sim, const tg_contact_frame *sensors, int32_t num_sensors, "
                         "const tg_imu_params *params, const float *bias, const int64_t *reset, float *history, "
                         "float *out)")
    from thormang_isaacgym_amd import abi
    for name in ("TG_IMU_MAX_SENSORS", "TG_IMU_WIDTH", "TG_IMU_HISTORY"):
        m = re.search(rf"^#define {name}\s+(\d+)\b", text, re.M)
        assert m and int(m.group(1)) == getattr(abi, name), name
    assert (abi.TG_IMU_MAX_SENSORS, abi.TG_IMU_WIDTH, abi.TG_IMU_HISTORY) == (8, 20, 8)


def test_struct_layout_matches_the_header():
    from thormang_isaacgym_amd import abi
    text = _header()
    body = text[text.index("typedef struct tg_imu_params {"):text.index("} tg_imu_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = {"int32_t": C.c_int32, "float": C.c_float, "uint64_t": C.c_uint64}
    assert [(n, want[t]) for n, t in fields] == list(abi.tg_imu_params._fields_)
    assert [n for n, _t in fields] == ["dt", "gyro_noise", "accel_noise", "pad", "seed", "counter"]
    assert C.sizeof(abi.tg_imu_params) == 32
    P = abi.tg_imu_params
    assert (P.dt.offset, P.gyro_noise.offset, P.accel_noise.offset, P.pad.offset, P.seed.offset,
            P.counter.offset) == (0, 4, 8, 12, 16, 24)


def test_header_index_has_the_entry():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_imu "):head.index("tg_get_sim_params")]
    assert "inertial measurement unit" in entry and "gyro" in entry and "accelerometer" in entry
    assert "tasks/gogoro_realistic_turning_sim_paper.py :55-67, :525-531" in entry


def test_header_fixes_the_definitions():
    text = _header()
    start, end = text.index("The inertial measurement unit in one kernel"), text.index("#define TG_IMU_MAX_SENSORS")
    body = _flat(text[start:end])
    for phrase in ("stream-ordered", "from the current root and dof state",
                   "the sim's gravity at the time of the call", "(tg_set_gravity is honoured)",
                   "nothing of the sim is written", "the library keeps nothing between calls",
                   "no host cache, no hidden step counter", "caller-owned history tensor",
                   "p_s = o_l + R_l offset_s", "a link may appear in several sensors", "Its axes are the link's",
                   "R = R_l", "w = the link's world angular velocity",
                   "v = the world velocity of the material point p_s",
                   "root_state[7:10] is the velocity of the root link's centre of mass",
                   "out[e, s, 0:TG_IMU_WIDTH]",
                   "0:4 the link's world quaternion xyzw, as tg_rigid_body_states reports it",
                   "4:7 gravity_b = R^T g / |g|, zero when |g| = 0", "7:10 lin_vel_b = R^T v",
                   "10:13 ang_vel_b = R^T w + bias[e, s, 0:3] + gyro_noise n[0:3]",
                   "13:16 lin_acc_b = R^T (a - g) + bias[e, s, 3:6] + accel_noise n[3:6]",
                   "the specific force: +|g| along world up at rest, 0 in free fall",
                   "16:19 ang_acc_b = R^T alpha", "19 valid: 1.0 where a and alpha were differenced, else 0.0",
                   "a = (v - v_prev) / dt and alpha = (w - w_prev) / dt", "history [N, S, TG_IMU_HISTORY]",
                   "v world in slots 0:3, w world in slots 3:6, the valid flag in slot 6, slot 7 written 0",
                   "a = alpha = 0 and valid = 0", "the accelerometer reads -R^T g",
                   "history is NULL, the history's flag is not 1.0, or reset[e] != 0",
                   "writes the current true (noise-free, bias-free) v, w and the flag 1.0 into history",
                   "reset envs included", "the history is read before it is written",
                   "dt is the sim time since the history was written; the caller states it",
                   "reset is [N] int64 on the device or NULL", "VecTask.reset_buf", "tg_walk_buffers.reset_buf",
                   "bias is [N, S, 6] on the device or NULL", "drawn only when a sigma is non-zero",
                   "Philox block 3 (e S + s) + j, j = 0..2", "counter (block, counter lo, counter hi, 0)",
                   "key seed", "gauss(x, y), gauss(z, w) are n[2j], n[2j+1]",
                   "tg_rng_fill kind 2 with n = 3 N S", "relative to the root link's origin",
                   "no absolute position enters any output", "Envs do not interact",
                   "Every element of out is written", "TG_ERR_ARG", "tg_imu: ...", "nothing launched",
                   "null sensors, params or out", "num_sensors outside 1..TG_IMU_MAX_SENSORS", "a negative link",
                   "a non-finite offset", "a non-finite or negative sigma",
                   "a history given with a dt that is not finite and > 0", "a null sim", "a link >= L",
                   "what needs no sim first, then the sim, then the links",
                   "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def _good():
    """Arguments no check objects to (the device pointers are never read by the host)."""
    from thormang_isaacgym_amd import abi
    sensors = (abi.tg_contact_frame * 2)()
    sensors[1].link = 3
    sensors[1].offset[:] = [0.1, -0.2, 0.3]
    ip = abi.tg_imu_params()
    ip.dt, ip.gyro_noise, ip.accel_noise, ip.seed, ip.counter = 0.01, 0.02, 0.3, 7, 9
    dev = C.c_void_p(0x1000)
    return dict(sensors=sensors, S=2, ip=ip, bias=dev, reset=dev, history=dev, out=dev)


def _call(a):
    from thormang_isaacgym_amd import _lib
    rc = _lib.lib().tg_imu(None, a["sensors"], a["S"], None if a["ip"] is None else C.byref(a["ip"]), a["bias"],
                           a["reset"], a["history"], a["out"])
    return rc, _lib.lib().tg_last_error().decode()


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_contact_frame), C.c_int32, C.POINTER(abi.tg_imu_params), C.c_void_p,
           C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["tg_imu"] == sig
    f = _lib.lib().tg_imu
    assert f.argtypes == sig and f.restype is C.c_int
    # good arguments and a null sim: the sim is rejected with a message, not dereferenced
    rc, msg = _call(_good())
    assert rc == -1 and msg.startswith("tg_imu: null tg_sim")   # TG_ERR_ARG


def _bad(**kw):
    a = _good()
    for k, v in kw.items():
        if k.startswith("ip_"):
            setattr(a["ip"], k[3:], v)
        elif k == "offset":
            a["sensors"][1].offset[2] = v
        elif k == "link":
            a["sensors"][0].link = v
        else:
            a[k] = v
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    ("null sensors", dict(sensors=None), "null sensors"),
    ("null params", dict(ip=None), "null params"),
    ("null out", dict(out=None), "null out"),
    ("no sensors", dict(S=0), "num_sensors 0 outside 1..8"),
    ("too many sensors", dict(S=9), "num_sensors 9 outside 1..8"),
    ("negative sensors", dict(S=-1), "num_sensors -1 outside 1..8"),
    ("negative link", dict(link=-1), "sensor 0: link -1"),
    ("nan offset", dict(offset=NAN), "sensor 1: offset[2] is not finite"),
    ("inf offset", dict(offset=INF), "sensor 1: offset[2] is not finite"),
    ("nan gyro sigma", dict(ip_gyro_noise=NAN), "gyro_noise"),
    ("inf gyro sigma", dict(ip_gyro_noise=INF), "gyro_noise"),
    ("negative gyro sigma", dict(ip_gyro_noise=-0.1), "gyro_noise"),
    ("nan accel sigma", dict(ip_accel_noise=NAN), "accel_noise"),
    ("negative accel sigma", dict(ip_accel_noise=-1.0), "accel_noise"),
    ("history with dt 0", dict(ip_dt=0.0), "history with a dt"),
    ("history with a negative dt", dict(ip_dt=-0.01), "history with a dt"),
    ("history with a nan dt", dict(ip_dt=NAN), "history with a dt"),
    ("history with an inf dt", dict(ip_dt=INF), "history with a dt"),
]


@pytest.mark.parametrize("name,change,text", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_are_reported_before_the_sim_is_looked_at(name, change, text):
    rc, msg = _call(_bad(**change))
    assert rc == -1, msg                                                     # TG_ERR_ARG
    assert msg.startswith("tg_imu: ") and text in msg and "null tg_sim" not in msg, msg


def test_the_checks_run_in_the_order_of_the_header():
    # two bad arguments: the earlier one in the header's list is the one reported
    order = [dict(sensors=None), dict(ip=None), dict(out=None), dict(S=0), dict(link=-1), dict(ip_gyro_noise=-1.0),
             dict(ip_dt=0.0)]
    texts = ["null sensors", "null params", "null out", "num_sensors", "link -1", "gyro_noise", "history with a dt"]
    for i in range(len(order) - 1):
        if "ip" in order[i] and order[i]["ip"] is None:
            later = dict(S=0)                      # (no params: nothing of them can be made bad as well)
            rc, msg = _call(_bad(**order[i], **later))
        else:
            rc, msg = _call(_bad(**order[i], **order[i + 1]))
        assert rc == -1 and texts[i] in msg, (i, msg)
    # a negative link of sensor 1 is found before a bad offset of sensor 1 only after sensor 0 passed: the loop runs
    # sensor by sensor, link first
    a = _bad(offset=NAN)
    a["sensors"][1].link = -2
    rc, msg = _call(a)
    assert rc == -1 and "sensor 1: link -2" in msg


def test_optional_arguments_and_unjudged_fields():
    ok = "tg_imu: null tg_sim"                                               # (only the sim is missing)
    rc, msg = _call(_bad(bias=None, reset=None, history=None))
    assert rc == -1 and msg.startswith(ok)
    # dt is not judged without a history
    for dt in (0.0, -1.0, NAN):
        rc, msg = _call(_bad(history=None, ip_dt=dt))
        assert rc == -1 and msg.startswith(ok), msg
    # zero sigmas are fine, and so is any seed or counter
    rc, msg = _call(_bad(ip_gyro_noise=0.0, ip_accel_noise=0.0, ip_seed=2 ** 64 - 1, ip_counter=2 ** 63))
    assert rc == -1 and msg.startswith(ok)


def test_python_layers_have_the_methods():
    from thormang_isaacgym_amd.sim import Imu, Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    want = [("sensors", inspect.Parameter.empty), ("history", None), ("dt", None), ("reset", None), ("bias", None),
            ("gyro_noise", 0.0), ("accel_noise", 0.0), ("seed", 0), ("counter", 0), ("out", None)]
    for cls in (Sim, VecTask):
        assert callable(getattr(cls, "imu")), cls.__name__
        got = [(p.name, p.default) for p in list(inspect.signature(cls.imu).parameters.values())[1:]]
        assert got == want, (cls.__name__, got)
    assert Imu._fields == ("quat", "gravity", "lin_vel", "ang_vel", "lin_acc", "ang_acc", "valid", "raw")
    assert [p for p in inspect.signature(Sim.imu_history).parameters][1:] == ["num_sensors"]


def test_walk_option_is_optional_and_off_in_the_shipped_configs():
    import yaml
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "tasks", "thormang_walk.py")) as f:
        src = f.read()
    assert '.get("enableImu", False)' in src and 'extras["imu"]' in src and '"imu_link"' in src
    assert "walk_post_kernel" in src and "taken before the step" in " ".join(src.split())
    cfg_dir = os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task")
    for name in os.listdir(cfg_dir):
        if name.endswith(".yaml"):
            with open(os.path.join(cfg_dir, name)) as f:
                assert "enableImu" not in (yaml.safe_load(f).get("env") or {}), name
    from thormang_isaacgym_amd.sim import load_model
    m = load_model("thormang")
    assert m.link_index("imu_link") == 27 and m.num_bodies == 44


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_imu" in line and "Sim.imu(" in line and "imu_history" in line and "enableImu" in line
               and "gogoro_realistic_turning_sim_paper.py" in line and line.lstrip().startswith("|")
               for line in text.splitlines())
