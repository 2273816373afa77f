"""The capsule proximity, its interface: the header declares tg_proximity,
tg_capsule (32 bytes), tg_proximity_params and the TG_PROX_* limits, has the
index entry and fixes the definitions; abi.py agrees with the header; the
library exports the symbol and the ctypes binding has its argument types; the
Python layers have the methods, the task option is optional and off in the
shipped configs, and INTEGRATION.md has the row.  The sim is the first argument
the call checks, so only the null sim can be judged without a device; every
other documented error is raised on a sim (marked gpu), in the header's order,
with its message, and with nothing launched: outputs filled with NaN stay NaN."""
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


def test_header_declares_the_entry_point_the_structs_and_the_limits():
    text = _header()
    assert re.search(r"^int\s+tg_proximity\(tg_sim \*sim,", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_proximity("):].split(";")[0], flags=re.S))
    decl = re.sub(r"\s+([,)])", r"\1", decl)
    assert decl == _flat("int tg_proximity(tg_sim *sim, const tg_capsule *capsules, int32_t num_capsules, "
                         "const int32_t *pairs, int32_t num_pairs, const tg_proximity_params *params, float *dist, "
                         "float *witness, float *summary)")
    from thormang_isaacgym_amd import abi
    for name in ("TG_PROX_MAX_CAPSULES", "TG_PROX_MAX_PAIRS"):
        m = re.search(rf"^#define {name}\s+(\d+)\b", text, re.M)
        assert m and int(m.group(1)) == getattr(abi, name), name
    assert (abi.TG_PROX_MAX_CAPSULES, abi.TG_PROX_MAX_PAIRS) == (32, 256)


def _fields(text, name):
    body = text[text.index(f"typedef struct {name} {{"):text.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            ctype, names = stmt.split(None, 1)
            out += [(n.strip(), ctype) for n in names.split(",")]
    return out


def test_struct_layouts_match_the_header():
    from thormang_isaacgym_amd import abi
    text = _header()
    assert _fields(text, "tg_capsule") == [("link", "int32_t"), ("p0[3]", "float"), ("p1[3]", "float"),
                                           ("radius", "float")]
    assert [n for n, _t in abi.tg_capsule._fields_] == ["link", "p0", "p1", "radius"]
    assert C.sizeof(abi.tg_capsule) == 32
    assert (abi.tg_capsule.link.offset, abi.tg_capsule.p0.offset, abi.tg_capsule.p1.offset,
            abi.tg_capsule.radius.offset) == (0, 4, 16, 28)
    assert _fields(text, "tg_proximity_params") == [("margin", "float")]
    assert list(abi.tg_proximity_params._fields_) == [("margin", C.c_float)] and C.sizeof(abi.tg_proximity_params) == 4


def test_header_index_and_definitions():
    text = _header()
    head = _flat(text[:text.index("#ifndef")])
    entry = head[head.index(" tg_proximity "):head.index("tg_get_sim_params")]
    assert "self-collision" in entry and "capsules" in entry and "summary" in entry
    body = _flat(text[text.index("Self-collision sensing in one kernel"):text.index("#define TG_PROX_MAX_CAPSULES")])
    for phrase in ("stream-ordered", "from the current root and dof state", "nothing of the sim is written",
                   "nothing is kept on the host between calls", "A NULL output is not touched",
                   "every element of every non-NULL output is written", "there is no contact response between links",
                   "x(s) = o_l + R_l (p0 + s (p1 - p0)), s in [0, 1]", "p0 == p1 is a sphere",
                   "Two capsules on the same link are allowed", "indices into capsules",
                   "the least distance between the two axis segments", "dist[e, p] = delta - r_a - r_b",
                   "a negative value is the penetration depth", "then one on axis b (3), in world coordinates",
                   "any minimiser may be returned", "[0] the smallest dist over the pairs",
                   "[1] the lowest pair index that attains it, as a float",
                   "[2] the number of pairs with dist < margin", "[3] sum_p max(0, margin - dist_p)",
                   "the root position is added last, and only to witness",
                   "dist and summary do not depend on where the env stands", "bit-reproducible from call to call",
                   "Envs do not interact", "forms no index from device data",
                   "TG_ERR_ARG", "tg_proximity: ...", "nothing launched", "a null sim",
                   "null capsules, pairs or params", "num_capsules outside 1..TG_PROX_MAX_CAPSULES",
                   "num_pairs outside 1..TG_PROX_MAX_PAIRS", "a link outside [0, L)",
                   "a non-finite end point or radius or a negative radius",
                   "a pair index outside [0, C) or a pair of a capsule with itself", "a non-finite margin",
                   "all three outputs NULL", "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def test_library_exports_and_binds_the_symbol_and_rejects_a_null_sim():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    sig = [C.c_void_p, C.POINTER(abi.tg_capsule), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
           C.POINTER(abi.tg_proximity_params), C.c_void_p, C.c_void_p, C.c_void_p]
    assert _lib.SIGNATURES["tg_proximity"] == sig
    f = _lib.lib().tg_proximity
    assert f.argtypes == sig and f.restype is C.c_int
    # the sim is judged first: with every other argument bad too, the message names the sim and nothing is read
    for args in ((None, 0, None, 0, None, None, None, None),
                 ((abi.tg_capsule * 2)(), 2, (C.c_int32 * 2)(0, 1), 1, abi.tg_proximity_params(), C.c_void_p(0x1000),
                  None, None)):
        rc = f(None, *args)
        assert rc == -1 and _lib.lib().tg_last_error().decode().startswith("tg_proximity: null tg_sim")


def test_python_layers_have_the_methods():
    from thormang_isaacgym_amd.sim import Proximity, Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    assert Proximity._fields == ("dist", "witness", "summary")
    for cls in (Sim, VecTask):
        got = [(p.name, p.default) for p in list(inspect.signature(cls.proximity).parameters.values())[1:]]
        assert [n for n, _d in got][:6] == ["capsules", "pairs", "margin", "dist", "witness", "summary"]
        assert [n for n, _d in got][6:] == ["out", "out_witness", "out_summary"]
        assert [d for _n, d in got][2:] == [0.0, True, False, False, None, None, None]
    sig = inspect.signature(Sim.capsule).parameters
    assert list(sig)[1:] == ["link", "p0", "p1", "radius"] and sig["p1"].default is None and sig["radius"].default == 0.05
    assert list(inspect.signature(Sim.limb_capsule).parameters)[1:] == ["link", "child", "radius"]
    sig = inspect.signature(Sim.capsule_pairs).parameters
    assert list(sig)[1:] == ["capsules", "min_hops"] and sig["min_hops"].default == 3


def test_walk_option_is_optional_and_off_in_the_shipped_configs():
    import yaml
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "tasks", "thormang_walk.py")) as f:
        src = f.read()
    assert '.get("enableSelfProximity", False)' in src and 'extras["self_proximity"]' in src
    assert '.get("selfProximityMargin", WALK_SELF_MARGIN)' in src
    cfg_dir = os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task")
    for name in os.listdir(cfg_dir):
        if name.endswith(".yaml"):
            with open(os.path.join(cfg_dir, name)) as f:
                env = yaml.safe_load(f).get("env") or {}
            assert "enableSelfProximity" not in env and "selfProximityMargin" not in env, name


def test_integration_table_has_a_row():
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        text = f.read()
    assert any("tg_proximity" in line and "proximity(" in line and "enableSelfProximity" in line
               and line.lstrip().startswith("|") for line in text.splitlines())


# ------------------------------------------------------------------ on a sim

NAN, INF = float("nan"), float("inf")
# (what is wrong, the change, a piece of the message), in the header's order
ERRORS = [
    ("null capsules", dict(caps=None), "null capsules"),
    ("null pairs", dict(pairs=None), "null pairs"),
    ("null params", dict(pp=None), "null params"),
    ("no capsules", dict(C=0), "num_capsules 0 outside 1..32"),
    ("too many capsules", dict(C=33), "num_capsules 33 outside 1..32"),
    ("negative capsules", dict(C=-1), "num_capsules -1 outside 1..32"),
    ("no pairs", dict(P=0), "num_pairs 0 outside 1..256"),
    ("too many pairs", dict(P=257), "num_pairs 257 outside 1..256"),
    ("negative link", dict(link=-1), "capsule 1: link -1 outside [0, "),
    ("link L", dict(link="L"), "capsule 1: link "),
    ("nan p0", dict(p0=NAN), "capsule 2: p0[1] is not finite"),
    ("inf p1", dict(p1=INF), "capsule 2: p1[2] is not finite"),
    ("nan radius", dict(radius=NAN), "capsule 0: radius nan"),
    ("inf radius", dict(radius=INF), "capsule 0: radius inf"),
    ("negative radius", dict(radius=-0.01), "capsule 0: radius -0.01"),
    ("pair index C", dict(pair=(1, 3)), "pair 1: (1, 3) outside [0, 3)"),
    ("negative pair index", dict(pair=(-1, 2)), "pair 1: (-1, 2) outside [0, 3)"),
    ("pair with itself", dict(pair=(2, 2)), "pair 1: capsule 2 with itself"),
    ("nan margin", dict(margin=NAN), "margin nan is not finite"),
    ("inf margin", dict(margin=INF), "margin inf is not finite"),
    ("no output", dict(dist=None, witness=None, summary=None), "dist, witness and summary are all null"),
]


class _Sim:
    def __init__(self):
        import torch
        from tests import physics_models as pm
        from thormang_isaacgym_amd.sim import Sim, load_model
        m = load_model("gogoro")
        self.n = 3
        self.s = Sim(m, pm.sim(m, n=self.n, dt=0.01, substeps=1)[1], self.n, "cuda:0")
        self.out = [torch.full(shape, NAN, dtype=torch.float32, device="cuda:0")
                    for shape in ((self.n, 2), (self.n, 2, 6), (self.n, 4))]

    def good(self):
        from thormang_isaacgym_amd import abi
        caps = (abi.tg_capsule * 3)()
        for k, c in enumerate(caps):
            c.link, c.radius = 3 * k, 0.05
            c.p1[:] = [0.1, 0.0, 0.2]
        pp = abi.tg_proximity_params()
        pp.margin = 0.02
        d, w, sm = (C.c_void_p(t.data_ptr()) for t in self.out)
        return dict(caps=caps, C=3, pairs=(C.c_int32 * 4)(0, 1, 1, 2), P=2, pp=pp, dist=d, witness=w, summary=sm)

    def bad(self, **kw):
        a = self.good()
        edits = ("link", "p0", "p1", "radius", "pair", "margin")            # (these first: an argument may become None)
        for k, v in sorted(kw.items(), key=lambda kv: kv[0] not in edits):
            if k == "link":
                a["caps"][1].link = self.s.L if v == "L" else v
            elif k == "p0":
                a["caps"][2].p0[1] = v
            elif k == "p1":
                a["caps"][2].p1[2] = v
            elif k == "radius":
                a["caps"][0].radius = v
            elif k == "pair":
                a["pairs"][2], a["pairs"][3] = v
            elif k == "margin":
                a["pp"].margin = v
            else:
                a[k] = v
        return a

    def call(self, a):
        from thormang_isaacgym_amd import _lib
        rc = _lib.lib().tg_proximity(self.s.handle, a["caps"], a["C"], a["pairs"], a["P"],
                                     None if a["pp"] is None else C.byref(a["pp"]), a["dist"], a["witness"],
                                     a["summary"])
        return rc, _lib.lib().tg_last_error().decode()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in self.out)


_sim = []


def _shared():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    if not _sim:
        _sim.append(_Sim())
    return _sim[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name,change,text", ERRORS, ids=[e[0] for e in ERRORS])
def test_argument_errors_have_their_messages_and_launch_nothing(name, change, text):
    t = _shared()
    rc, msg = t.call(t.bad(**change))
    assert rc == -1, msg                                                     # TG_ERR_ARG
    assert msg.startswith("tg_proximity: ") and text in msg, msg
    assert t.untouched()


@pytest.mark.gpu
def test_errors_come_in_the_headers_order():
    """Two bad arguments: the one the header lists first is reported."""
    t = _shared()
    order = [dict(caps=None), dict(pp=None), dict(C=0), dict(P=0), dict(link=-1), dict(radius=-1.0),
             dict(pair=(2, 2)), dict(margin=NAN), dict(dist=None, witness=None, summary=None)]
    texts = ["null capsules", "null params", "num_capsules", "num_pairs", "link -1", "radius -1", "with itself",
             "margin nan", "all null"]
    for k in range(len(order) - 1):
        for j in range(k + 1, len(order)):
            rc, msg = t.call(t.bad(**order[k], **order[j]))
            assert rc == -1 and texts[k] in msg and texts[j] not in msg, msg
    # a link outside the model is reported before a non-finite end point of an earlier capsule
    a = t.bad(link="L")
    a["caps"][0].p0[0] = NAN
    rc, msg = t.call(a)
    assert rc == -1 and "capsule 1: link" in msg, msg
    assert t.untouched()


@pytest.mark.gpu
def test_accepted_calls_write_every_element():
    import torch
    t = _shared()
    from thormang_isaacgym_amd import abi
    own = [torch.full_like(o, NAN) for o in t.out]                          # (t.out stays NaN for the error tests)
    ptr = dict(zip(("dist", "witness", "summary"), (C.c_void_p(o.data_ptr()) for o in own)))
    for keep in ptr:
        rc, msg = t.call(t.bad(**{k: (v if k == keep else None) for k, v in ptr.items()}))
        assert rc == 0, msg
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in own) and t.untouched()
    # two capsules on one link, a sphere among them, and the limits of both counts
    a = t.good()
    a["caps"] = (abi.tg_capsule * 32)()
    for k, c in enumerate(a["caps"]):
        c.link, c.radius = k % 2, 0.0
        c.p0[:] = [0.01 * k, 0.0, 0.0]
        c.p1[:] = [0.01 * k, 0.0, 0.1 * (k % 3)]
    a["C"], a["P"] = 32, 256
    a["pairs"] = (C.c_int32 * 512)(*[v for k in range(256) for v in (k % 32, (k % 32 + 1 + k // 32) % 32)])
    big = [torch.full(shape, NAN, dtype=torch.float32, device="cuda:0") for shape in ((t.n, 256), (t.n, 256, 6))]
    a["dist"], a["witness"], a["summary"] = C.c_void_p(big[0].data_ptr()), C.c_void_p(big[1].data_ptr()), ptr["summary"]
    rc, msg = t.call(a)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(x).all()) for x in big)
