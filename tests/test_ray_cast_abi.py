"""The ray cast, the parts that need no GPU: the header declares tg_ray_cast,
tg_ray_params and the TG_RAY_* constants, has the index entry and fixes the
definitions; abi.py agrees with the header; the library exports the symbol and
the ctypes binding has its argument types; every argument error that can be
judged without a sim is raised, in the header's order -- the call checks its
arguments before it looks at the sim, so a null sim with one bad argument
reports the argument, and a null sim with good arguments reports the sim:
nothing can have been launched -- the Python layers have the methods, the task
option is optional and off in the shipped config, and INTEGRATION.md has the
row.  (A link >= L needs a sim: tests/test_gpu_ray_cast.py.)"""
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
    assert re.search(r"^int\s+tg_ray_cast\(tg_sim \*sim,", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_ray_cast("):].split(";")[0], flags=re.S))
    decl = re.sub(r"\s+([,)])", r"\1", decl)           # (a comment may stand between a name and its comma)
    assert decl == _flat("int tg_ray_cast(tg_sim *sim, const tg_contact_frame *frames, int32_t num_frames, "
                         "const float *rays, int32_t num_rays, const tg_ray_params *params, float *dist, "
                         "float *normals)")
    from thormang_isaacgym_amd import abi
    for name in ("TG_RAY_MAX_FRAMES", "TG_RAY_MAX_RAYS", "TG_RAY_LINK", "TG_RAY_YAW", "TG_RAY_WORLD"):
        m = re.search(rf"^#define {name}\s+(\d+)\b", text, re.M)
        assert m and int(m.group(1)) == getattr(abi, name), name
    assert (abi.TG_RAY_MAX_FRAMES, abi.TG_RAY_MAX_RAYS) == (8, 4096)
    assert (abi.TG_RAY_LINK, abi.TG_RAY_YAW, abi.TG_RAY_WORLD) == (0, 1, 2)


def test_struct_layout_matches_the_header():
    from thormang_isaacgym_amd import abi
    text = _header()
    body = text[text.index("typedef struct tg_ray_params {"):text.index("} tg_ray_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    want = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, want[t]) for n, t in fields] == list(abi.tg_ray_params._fields_)
    assert [n for n, _t in fields] == ["align", "max_range"]
    assert C.sizeof(abi.tg_ray_params) == 8
    assert abi.tg_ray_params.align.offset == 0 and abi.tg_ray_params.max_range.offset == 4


def test_header_index_has_the_entry():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_ray_cast "):head.index("tg_get_sim_params")]
    assert "lidar" in entry and "depth-camera" in entry and "heightfield" in entry


def test_header_fixes_the_definitions():
    text = _header()
    body = _flat(text[text.index("Range sensing in one kernel"):text.index("#define TG_RAY_MAX_FRAMES")])
    for phrase in ("stream-ordered", "from the current root and dof state",
                   "the heightfield the sim holds at the time of the call", "removal with rows = 0 included",
                   "is seen by the next call", "nothing of the sim is written",
                   "nothing is kept on the host between calls", "A NULL output is not touched",
                   "every element of every non-NULL output is written",
                   "p_f = o_l + R_l offset_f", "as in tg_height_scan", "a link may appear in several frames",
                   "rays[k] = (s_k, d_k)", "one pattern for every env and frame",
                   "TG_RAY_LINK A = R_l", "TG_RAY_YAW A = Rz(psi)",
                   "(cos psi, sin psi) is (R00 + R11, R10 - R01) normalised", "the identity when both are 0",
                   "TG_RAY_WORLD A = I", "x(t) = p_f + A s_k + t A d_k, t >= 0", "d_k is NOT normalised",
                   "t is the ray parameter", "with unit directions t is the range", "scaled to d.x = 1",
                   "max_range bounds t", "the fu >= fv rule of ground_at", "the closed grid rectangle",
                   "G = {z <= 0} u {(x, y) on the grid and z <= H(x, y)}",
                   "dist[e, f, k] = inf {t in [0, max_range] : x(t) in G}", "max_range exactly", "(a miss)",
                   "iff dist < max_range", "e_z when the half-space z <= 0 is entered first",
                   "the x face wins at a corner", "(+-1, 0, 0), (0, +-1, 0)", "starts inside G (dist = 0)",
                   "(0, 0, 0) on a miss", "zero or non-finite direction or start", "non-finite state, reads a miss",
                   "the root position is added last", "agrees with tg_rigid_body_states to rounding",
                   "Envs do not interact", "bounded by rows + cols + 4 cells",
                   "TG_ERR_ARG", "tg_ray_cast: ...", "nothing launched", "null frames, rays or params",
                   "dist and normals both NULL", "num_frames outside 1..TG_RAY_MAX_FRAMES",
                   "num_rays outside 1..TG_RAY_MAX_RAYS", "a negative link", "a non-finite offset",
                   "align outside {0, 1, 2}", "max_range that is not finite and > 0", "a null sim", "a link >= L",
                   "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def _good():
    """Arguments no check objects to (the device pointers are never read by the host)."""
    from thormang_isaacgym_amd import abi
    frames = (abi.tg_contact_frame * 2)()
    frames[1].link = 3
    frames[1].offset[:] = [0.1, -0.2, 0.3]
    rp = abi.tg_ray_params()
    rp.align, rp.max_range = abi.TG_RAY_LINK, 8.0
    dev = C.c_void_p(0x1000)
    return dict(frames=frames, F=2, rays=dev, R=96, rp=rp, dist=dev, normals=dev)


def _call(a):
    from thormang_isaacgym_amd import _lib
    rc = _lib.lib().tg_ray_cast(None, a["frames"], a["F"], a["rays"], a["R"],
                                None if a["rp"] is None else C.byref(a["rp"]), a["dist"], a["normals"])
    return rc, _lib.lib().tg_last_error().decode()


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_contact_frame), C.c_int32, C.c_void_p, C.c_int32,
           C.POINTER(abi.tg_ray_params), C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["tg_ray_cast"] == sig
    f = _lib.lib().tg_ray_cast
    assert f.argtypes == sig and f.restype is C.c_int
    # good arguments and a null sim: the sim is rejected with a message, not dereferenced
    rc, msg = _call(_good())
    assert rc == -1 and msg.startswith("tg_ray_cast: null tg_sim")   # TG_ERR_ARG


def _bad(**kw):
    a = _good()
    for k, v in kw.items():
        if k.startswith("rp_"):
            setattr(a["rp"], k[3:], v)
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
    ("null rays", dict(rays=None), "null rays"),
    ("null params", dict(rp=None), "null params"),
    ("no output", dict(dist=None, normals=None), "dist and normals are both null"),
    ("no frames", dict(F=0), "num_frames 0 outside 1..8"),
    ("too many frames", dict(F=9), "num_frames 9 outside 1..8"),
    ("negative frames", dict(F=-1), "num_frames -1 outside 1..8"),
    ("no rays", dict(R=0), "num_rays 0 outside 1..4096"),
    ("too many rays", dict(R=4097), "num_rays 4097 outside 1..4096"),
    ("negative link", dict(link=-1), "frame 0: link -1"),
    ("nan offset", dict(offset=NAN), "frame 1: offset[2] is not finite"),
    ("inf offset", dict(offset=INF), "frame 1: offset[2] is not finite"),
    ("align 3", dict(rp_align=3), "align 3"),
    ("align -1", dict(rp_align=-1), "align -1"),
    ("zero range", dict(rp_max_range=0.0), "max_range 0"),
    ("negative range", dict(rp_max_range=-2.0), "max_range -2"),
    ("inf range", dict(rp_max_range=INF), "max_range inf"),
    ("nan range", dict(rp_max_range=NAN), "max_range"),
]


@pytest.mark.parametrize("name,change,text", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_are_reported_before_the_sim_is_looked_at(name, change, text):
    rc, msg = _call(_bad(**change))
    assert rc == -1, msg                                                     # TG_ERR_ARG
    assert msg.startswith("tg_ray_cast: ") and text in msg and "null tg_sim" not in msg, msg


def test_errors_come_in_the_headers_order():
    """Two bad arguments: the one the header lists first is reported."""
    order = [dict(frames=None), dict(dist=None, normals=None), dict(F=0), dict(R=0), dict(link=-1),
             dict(rp_align=7), dict(rp_max_range=0.0)]
    texts = ["null frames", "both null", "num_frames", "num_rays", "link -1", "align 7", "max_range"]
    for k in range(len(order) - 1):
        rc, msg = _call(_bad(**order[k], **order[k + 1]))
        assert rc == -1 and texts[k] in msg and texts[k + 1] not in msg, msg


def test_one_output_alone_is_accepted():
    for change in (dict(dist=None), dict(normals=None), dict(rp_align=2), dict(rp_align=1), dict(R=4096), dict(F=8)):
        a = _bad(**change)
        if change.get("F") == 8:
            from thormang_isaacgym_amd import abi
            a["frames"] = (abi.tg_contact_frame * 8)()
        rc, msg = _call(a)
        assert rc == -1 and msg.startswith("tg_ray_cast: null tg_sim"), msg   # (only the sim is missing)


def test_python_layers_have_the_methods():
    from thormang_isaacgym_amd.sim import RayCast, Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    for cls in (Sim, VecTask):
        assert callable(getattr(cls, "ray_cast")), cls.__name__
        got = [(p.name, p.default) for p in list(inspect.signature(cls.ray_cast).parameters.values())[1:]]
        assert [n for n, _d in got] == ["frames", "rays", "align", "max_range", "normals", "out", "out_normals"]
        assert dict(got)["align"] == "link" and dict(got)["normals"] is False and dict(got)["out"] is None
    assert RayCast._fields == ("dist", "normals")
    assert [p for p in inspect.signature(Sim.lidar_rays).parameters][1:] == ["azimuths", "elevations"]
    assert [p for p in inspect.signature(Sim.pinhole_rays).parameters][1:] == ["width", "height", "hfov"]


def test_gogoro_option_is_optional_and_off_in_the_shipped_configs():
    import yaml
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "tasks", "gogoro.py")) as f:
        src = f.read()
    assert '.get("enableDepthCamera", False)' in src and 'extras["depth"]' in src
    cfg_dir = os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task")
    for name in os.listdir(cfg_dir):
        if name.endswith(".yaml"):
            with open(os.path.join(cfg_dir, name)) as f:
                assert "enableDepthCamera" not in (yaml.safe_load(f).get("env") or {}), name


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_ray_cast" in line and "ray_cast(" in line and "enableDepthCamera" in line
               and line.lstrip().startswith("|") for line in text.splitlines())
