"""The height scan, the parts that need no GPU: the header declares
tg_height_scan, tg_scan_params and the TG_SCAN_* constants, has the index entry
and fixes the definitions; abi.py agrees with the header; the library exports
the symbol and the ctypes binding has its argument types; every argument error
that can be judged without a sim is raised -- the call checks its arguments
before it looks at the sim, so a null sim with one bad argument reports the
argument, and a null sim with good arguments reports the sim: nothing can have
been launched -- the Python layers have the methods, the task option is
optional and off in the shipped config, and INTEGRATION.md has the row.  (A
link >= L needs a sim: tests/test_gpu_height_scan.py.)"""
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
    assert re.search(r"^int\s+tg_height_scan\(tg_sim \*sim,", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_height_scan("):].split(";")[0], flags=re.S))
    decl = re.sub(r"\s+([,)])", r"\1", decl)           # (a comment may stand between a name and its comma)
    assert decl == _flat("int tg_height_scan(tg_sim *sim, const tg_contact_frame *frames, int32_t num_frames, "
                         "const float *points, int32_t num_points, const tg_scan_params *params, float *heights, "
                         "float *normals)")
    from thormang_isaacgym_amd import abi
    for name in ("TG_SCAN_MAX_FRAMES", "TG_SCAN_MAX_POINTS", "TG_SCAN_SURFACE", "TG_SCAN_CELL", "TG_SCAN_YAW",
                 "TG_SCAN_WORLD", "TG_SCAN_LINK"):
        m = re.search(rf"^#define {name}\s+(\d+)\b", text, re.M)
        assert m and int(m.group(1)) == getattr(abi, name), name
    assert (abi.TG_SCAN_MAX_FRAMES, abi.TG_SCAN_MAX_POINTS) == (8, 1024)
    assert (abi.TG_SCAN_SURFACE, abi.TG_SCAN_CELL) == (0, 1)
    assert (abi.TG_SCAN_YAW, abi.TG_SCAN_WORLD, abi.TG_SCAN_LINK) == (0, 1, 2)


def test_struct_layout_matches_the_header():
    from thormang_isaacgym_amd import abi
    text = _header()
    body = text[text.index("typedef struct tg_scan_params {"):text.index("} tg_scan_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, want[t]) for n, t in fields] == list(abi.tg_scan_params._fields_)
    assert [n for n, _t in fields] == ["surface", "align", "relative", "bias", "lo", "hi", "scale"]
    assert C.sizeof(abi.tg_scan_params) == 28
    assert abi.tg_scan_params.bias.offset == 12 and abi.tg_scan_params.scale.offset == 24


def test_header_index_has_the_entry():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_height_scan "):head.index("tg_get_sim_params")]
    assert "measured_heights" in entry and "get_heights" in entry and "quat_apply_yaw" in entry
    assert "anymal_terrain.py:501-536" in entry


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("The ground under the robot in one kernel"):text.index("#define TG_SCAN_MAX_FRAMES")])
    for phrase in ("stream-ordered", "from the current root and dof state",
                   "the heightfield the sim holds at the time of the call", "removal with rows = 0 included",
                   "is seen by the next call", "nothing of the sim is written",
                   "nothing is kept on the host between calls", "A NULL output is not touched",
                   "every element of every non-NULL output is written",
                   "p_f = o_l + R_l offset_f", "tg_contact_frame, tg_set_force_sensor_tensor and tg_ik_chain.offset",
                   "those of tg_rigid_body_states", "a link may appear in several frames",
                   "(x, y) = (p_f.x, p_f.y) + d.xy", "TG_SCAN_WORLD d = (a, b, 0)", "TG_SCAN_LINK d = R_l (a, b, 0)",
                   "TG_SCAN_YAW d = Rz(psi) (a, b, 0)", "quat_apply_yaw", "with x and y zeroed, normalised",
                   "(cos psi, sin psi) is (R00 + R11, R10 - R01) normalised", "the identity when both are 0",
                   "TG_SCAN_SURFACE the surface the contacts feel", "(ground_at)", "whichever is higher",
                   "the plane outside the grid", "Without a heightfield h = 0 and n = e_z",
                   "TG_SCAN_CELL the reference's rule (anymal_terrain.py:524-536)", "u = (x - ox) / hs",
                   "i = clamp(trunc(u), 0, rows - 2)", "h = vs min(hf[i][j], hf[i+1][j+1])", "No plane",
                   "reads the border cell", "Without a heightfield h = 0", "normals must be NULL",
                   "heights[e, f, k] = h with params.relative == 0",
                   "heights[e, f, k] = clamp(p_f.z - bias - h, lo, hi) scale", "line 302 of the reference",
                   "the root position is added last", "agrees with tg_rigid_body_states to rounding",
                   "TG_ERR_ARG", "tg_height_scan: ...", "a null sim, frames, points or params",
                   "num_frames outside 1..TG_SCAN_MAX_FRAMES", "num_points outside 1..TG_SCAN_MAX_POINTS",
                   "a link outside [0, L)", "a non-finite offset", "surface outside {0, 1}", "align outside {0, 1, 2}",
                   "non-finite bias or scale", "lo <= hi", "normals together with TG_SCAN_CELL",
                   "heights and normals both NULL", "A rejected call launches nothing",
                   "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def _good():
    """Arguments no check objects to (the device pointers are never read by the host)."""
    from thormang_isaacgym_amd import abi
    frames = (abi.tg_contact_frame * 2)()
    frames[1].link = 3
    frames[1].offset[:] = [0.1, -0.2, 0.3]
    sp = abi.tg_scan_params()
    sp.surface, sp.align, sp.relative = abi.TG_SCAN_SURFACE, abi.TG_SCAN_YAW, 1
    sp.bias, sp.lo, sp.hi, sp.scale = 0.5, -1.0, 1.0, 5.0
    dev = C.c_void_p(0x1000)
    return dict(frames=frames, F=2, points=dev, P=140, sp=sp, heights=dev, normals=dev)


def _call(a):
    from thormang_isaacgym_amd import _lib
    rc = _lib.lib().tg_height_scan(None, a["frames"], a["F"], a["points"], a["P"],
                                   None if a["sp"] is None else C.byref(a["sp"]), a["heights"], a["normals"])
    return rc, _lib.lib().tg_last_error().decode()


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_contact_frame), C.c_int32, C.c_void_p, C.c_int32,
           C.POINTER(abi.tg_scan_params), C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["tg_height_scan"] == sig
    f = _lib.lib().tg_height_scan
    assert f.argtypes == sig and f.restype is C.c_int
    # good arguments and a null sim: the sim is rejected with a message, not dereferenced
    rc, msg = _call(_good())
    assert rc == -1 and msg.startswith("tg_height_scan: null tg_sim")   # TG_ERR_ARG


def _bad(**kw):
    a = _good()
    for k, v in kw.items():
        if k.startswith("sp_"):
            setattr(a["sp"], k[3:], v)
        elif k == "offset":
            a["frames"][1].offset[2] = v
        elif k == "link":
            a["frames"][0].link = v
        else:
            a[k] = v
    return a


NAN, INF = float("nan"), float("inf")
ERRORS = [
    ("null frames", dict(frames=None), "null frames"),
    ("null points", dict(points=None), "null points"),
    ("null params", dict(sp=None), "null params"),
    ("no frames", dict(F=0), "num_frames 0 outside 1..8"),
    ("too many frames", dict(F=9), "num_frames 9 outside 1..8"),
    ("negative frames", dict(F=-1), "num_frames -1 outside 1..8"),
    ("no points", dict(P=0), "num_points 0 outside 1..1024"),
    ("too many points", dict(P=1025), "num_points 1025 outside 1..1024"),
    ("negative link", dict(link=-1), "frame 0: link -1"),
    ("nan offset", dict(offset=NAN), "frame 1: offset[2] is not finite"),
    ("inf offset", dict(offset=INF), "frame 1: offset[2] is not finite"),
    ("surface 2", dict(sp_surface=2), "surface 2"),
    ("surface -1", dict(sp_surface=-1), "surface -1"),
    ("align 3", dict(sp_align=3), "align 3"),
    ("align -1", dict(sp_align=-1), "align -1"),
    ("nan bias", dict(sp_bias=NAN), "non-finite bias"),
    ("inf scale", dict(sp_scale=INF), "non-finite bias"),
    ("lo > hi", dict(sp_lo=1.5), "lo <= hi"),
    ("normals with the cell rule", dict(sp_surface=1), "TG_SCAN_CELL has no normals"),
    ("no output", dict(heights=None, normals=None), "heights and normals are both null"),
]


@pytest.mark.parametrize("name,change,text", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_are_reported_before_the_sim_is_looked_at(name, change, text):
    rc, msg = _call(_bad(**change))
    assert rc == -1, msg                                                     # TG_ERR_ARG
    assert msg.startswith("tg_height_scan: ") and text in msg and "null tg_sim" not in msg, msg


def test_relative_fields_are_not_judged_without_relative():
    rc, msg = _call(_bad(sp_relative=0, sp_bias=NAN, sp_scale=INF, sp_lo=2.0, sp_hi=1.0))
    assert rc == -1 and msg.startswith("tg_height_scan: null tg_sim")        # (only the sim is missing)
    rc, msg = _call(_bad(sp_surface=1, normals=None))                        # the cell rule without normals is fine
    assert rc == -1 and msg.startswith("tg_height_scan: null tg_sim")
    rc, msg = _call(_bad(heights=None))                                      # normals alone too
    assert rc == -1 and msg.startswith("tg_height_scan: null tg_sim")
    rc, msg = _call(_bad(sp_lo=-INF, sp_hi=INF))                             # an open clamp
    assert rc == -1 and msg.startswith("tg_height_scan: null tg_sim")


def test_python_layers_have_the_methods():
    from thormang_isaacgym_amd.sim import HeightScan, Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    want = [("frames", inspect.Parameter.empty), ("points", inspect.Parameter.empty), ("surface", "surface"),
            ("align", "yaw"), ("normals", False), ("relative", None), ("out", None), ("out_normals", None)]
    for cls in (Sim, VecTask):
        assert callable(getattr(cls, "height_scan")), cls.__name__
        got = [(p.name, p.default) for p in list(inspect.signature(cls.height_scan).parameters.values())[1:]]
        assert got == want, (cls.__name__, got)
    assert HeightScan._fields == ("heights", "normals")
    assert [p for p in inspect.signature(Sim.scan_grid).parameters][1:] == ["xs", "ys"]


def test_gogoro_option_is_optional_and_off_in_the_shipped_configs():
    import yaml
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "tasks", "gogoro.py")) as f:
        src = f.read()
    assert '.get("enableHeightScan", False)' in src and 'extras["measured_heights"]' in src
    cfg_dir = os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task")
    for name in os.listdir(cfg_dir):
        if name.endswith(".yaml"):
            with open(os.path.join(cfg_dir, name)) as f:
                assert "enableHeightScan" not in (yaml.safe_load(f).get("env") or {}), name


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_height_scan" in line and "get_heights" in line and "init_height_points" in line
               and "height_scan(" in line and "enableHeightScan" in line and line.lstrip().startswith("|")
               for line in text.splitlines())
