"""The contact force distribution, its interface: the header declares
tg_contact_qp and TG_QP_MAX_ITERS, has the index entry and fixes the definition
and the algorithm; abi.py mirrors the constant and the defaults; the library
exports the symbol, the ctypes binding has its argument types, a null sim is
rejected; Sim.contact_qp and walk_sole_patch have their signatures.  On a sim
(marked gpu): every argument error has its message and launches nothing."""
import ctypes as C
import inspect
import os
import re

import pytest

from thormang_isaacgym_amd.sim import ContactForces, Sim          # (the feature: this file fails without it)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(REPO, "include", "tgsim.h")) as f:
        return f.read()


def _flat(s):
    return " ".join(s.replace("*", " ").split())


def test_header_declares_the_entry_point_and_the_constant():
    from thormang_isaacgym_amd import abi
    text = _header()
    assert re.search(r"^int\s+tg_contact_qp\(tg_sim \*sim, const tg_contact_frame \*contacts", text, re.M)
    decl = _flat(re.sub(r"/\*.*?\*/", "", text[text.index("int tg_contact_qp("):].split(";")[0], flags=re.S))
    assert decl == _flat("int tg_contact_qp(tg_sim *sim, const tg_contact_frame *contacts , int32_t num_contacts, "
                         "const float *extents , const float *normals , const float *friction , float mu, "
                         "const float *share , float moment_arm, float reg, float rho, float relax, int32_t iters, "
                         "int32_t terms, const float *accel , float *tau , float *wrench , float *forces , "
                         "float *info , float *efforts , const int32_t *dofs , int32_t num_dofs, int32_t accumulate)")
    mx = re.search(r"^#define TG_QP_MAX_ITERS\s+(\d+)\b", text, re.M)
    assert mx and int(mx.group(1)) == abi.TG_QP_MAX_ITERS == 256
    assert abi.TG_QP_DEFAULTS == {"reg": 0.03, "rho": 0.6, "relax": 1.6, "iters": 64}


def test_header_index_has_the_entry():
    head = _flat(_header()[:_header().index("#ifndef")])
    entry = head[head.index(" tg_contact_qp "):head.index("tg_get_sim_params")]
    assert "friction cones" in entry and "sole outlines" in entry and "ADMM" in entry and "cannot supply" in entry


def test_header_fixes_the_definition_and_the_algorithm():
    text = _header()
    body = _flat(text[text.index("Contact forces inside friction cones and sole outlines in one kernel launch"):
                      text.index("#define TG_QP_MAX_ITERS")])
    for phrase in ("are those of tg_contact_inverse_dynamics",
                   "p_kv = o_l + R_l (offset_k + (+-hx_k, +-hy_k, 0))", "(+,+), (+,-), (-,-), (-,+)",
                   "zero extents give a point contact", "J = 4 K vertex forces",
                   "C_k = { f : f.n_k >= 0, |f - (f.n_k) n_k| <= mu_k f.n_k }", "normalised in the kernel",
                   "a vector shorter than 1e-6 gives world z", "NULL gives world z",
                   "negative and NaN values are taken as 0", "G_kv = [1; [r_kv]x]",
                   "minimise 1/2 |b[0:6] - sum G_kv f_kv|^2_W + 1/2 reg sum_k (1/s_k) sum_v |f_kv|^2 over f_kv in C_k",
                   "exactly 0.0", "equal those of a call without it", "makes no iterations", "The balance is soft",
                   "the nearest feasible one", "ADMM in scaled form from z = u = 0", "P = diag(reg / s_k + rho)",
                   "c = G^T W b[0:6]", "q = c + rho (z - u)",
                   "x = P^-1 q - P^-1 G^T (W^-1 + G P^-1 G^T)^-1 G P^-1 q", "xh = relax x + (1 - relax) z",
                   "z = proj_C(xh + u)", "mu |t| <= -w_n: 0", "a = (mu |t| + w_n) / (1 + mu^2)", "u = u + xh - z",
                   "lies in its cone by construction", "reg = 0.03, rho = 0.6, relax = 1.6 and iters = 64",
                   "forces[e, k, v] = f_kv", "sum_v (p_kv - p_k) x f_kv", "the force sensor tensor",
                   "tau[6 + d] = b[6 + d] - sum_k Jp_k[:, 6 + d]^T wrench_k",
                   "the wrench the ground cannot supply", "the number of vertices with f.n > 0",
                   "Every element of every non-NULL output is written", "nothing of the sim is written",
                   "bit-identical wherever the env sits on the grid", "tg_contact_qp: ...", "null extents",
                   "an extent not finite or < 0", "mu not finite or < 0", "reg or rho not finite or <= 0",
                   "relax outside (0, 2)", "iters outside 1..TG_QP_MAX_ITERS",
                   "tau, wrench, forces, info and efforts all NULL", "every argument error of tg_inverse_dynamics",
                   "A rejected call launches nothing", "run-time (tg_model_jit) ones included"):
        assert phrase in body, phrase


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib, abi
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    VP, F, I = C.c_void_p, C.c_float, C.c_int32
    sig = [VP, C.POINTER(abi.tg_contact_frame), I, C.POINTER(F), VP, VP, F, VP, F, F, F, F, I, I, VP, VP, VP, VP, VP,
           VP, C.POINTER(I), I, I]
    assert _lib.SIGNATURES["tg_contact_qp"] == sig
    f = _lib.lib().tg_contact_qp
    assert f.argtypes == sig and f.restype is C.c_int
    frames, ext = (abi.tg_contact_frame * 1)(), (F * 2)()
    assert f(None, frames, 1, ext, None, None, 0.7, None, 0.1, 0.03, 0.6, 1.6, 64, 3, None, None, None, None, None,
             None, None, 0, 0) == -1                                         # TG_ERR_ARG, not dereferenced
    assert _lib.lib().tg_last_error().startswith(b"tg_contact_qp: null tg_sim")


def test_sim_and_the_walk_task_have_the_methods():
    from thormang_isaacgym_amd.sim import load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_centre, walk_sole_patch
    E = inspect.Parameter.empty
    want = [("contacts", E), ("extents", E), ("mu", 0.7), ("friction", None), ("normals", None), ("share", None),
            ("accel", None), ("gravity", True), ("velocity", True), ("moment_arm", 0.1), ("reg", 0.03), ("rho", 0.6),
            ("relax", 1.6), ("iters", 64), ("forces", False), ("info", False), ("efforts", None), ("dofs", None),
            ("accumulate", False)]
    got = [(p.name, p.default) for p in list(inspect.signature(Sim.contact_qp).parameters.values())[1:]]
    assert got == want, got
    assert ContactForces._fields == ("tau", "wrench", "forces", "info")
    m = load_model("thormang")
    for l in walk_feet_indices(m):
        off, (hx, hy) = walk_sole_patch(m, l)
        assert off == walk_sole_centre(m, l) and (hx, hy) == (0.11, 0.075)   # the sole: 0.22 m long, 0.15 m wide


# ------------------------------------------------------------------ on a sim

NAN, INF = float("nan"), float("inf")
# (what is wrong, the change, a piece of the message), in the header's order
ERRORS = [
    ("null contacts", dict(contacts=None), "null contacts"),
    ("null extents", dict(extents=None), "null extents"),
    ("no contacts", dict(K=0), "num_contacts 0 outside 1..4"),
    ("five contacts", dict(K=5), "num_contacts 5 outside 1..4"),
    ("negative link", dict(link=-1), "contact 1: link -1 outside [0, "),
    ("link L", dict(link="L"), "contact 1: link "),
    ("link twice", dict(link="same"), "appears twice"),
    ("negative extent", dict(ext=-0.01), "contact 1: extent[0] -0.01"),
    ("nan extent", dict(ext=NAN), "contact 1: extent[0] nan"),
    ("inf extent", dict(ext=INF), "contact 1: extent[0] inf"),
    ("negative mu", dict(mu=-0.1), "mu -0.1"),
    ("nan mu", dict(mu=NAN), "mu nan"),
    ("inf mu", dict(mu=INF), "mu inf"),
    ("moment_arm 0", dict(arm=0.0), "moment_arm 0"),
    ("moment_arm nan", dict(arm=NAN), "moment_arm nan"),
    ("reg 0", dict(reg=0.0), "reg 0"),
    ("reg inf", dict(reg=INF), "reg inf"),
    ("rho negative", dict(rho=-1.0), "rho -1"),
    ("rho nan", dict(rho=NAN), "rho nan"),
    ("relax 0", dict(relax=0.0), "relax 0 outside (0, 2)"),
    ("relax 2", dict(relax=2.0), "relax 2 outside (0, 2)"),
    ("relax nan", dict(relax=NAN), "relax nan outside (0, 2)"),
    ("iters 0", dict(iters=0), "iters 0 outside 1..256"),
    ("iters 257", dict(iters=257), "iters 257 outside 1..256"),
    ("terms 4", dict(terms=4), "terms 4 outside 0..3"),
    ("no terms, no accel", dict(terms=0), "no terms and no accel"),
    ("no output", dict(tau=None, wrench=None, forces=None, info=None, efforts=None), "are all null"),
    ("num_dofs negative", dict(num=-1), "num_dofs -1 outside"),
    ("null dofs", dict(num=2), "null dofs with num_dofs 2"),
    ("dof D", dict(dofs="D"), "outside [0, "),
    ("dof twice", dict(dofs=[1, 2, 1]), "DOF 1 appears twice"),
]


class _Sim:
    def __init__(self):
        import torch
        from tests import physics_models as pm
        from thormang_isaacgym_amd.sim import load_model
        m = load_model("gogoro")
        self.n = 3
        self.s = Sim(m, pm.sim(m, n=self.n, dt=0.01, substeps=1)[1], self.n, "cuda:0")
        D = self.s.D
        self.out = {k: torch.full(shape, NAN, dtype=torch.float32, device="cuda:0")
                    for k, shape in (("tau", (self.n, 6 + D)), ("wrench", (self.n, 2, 6)), ("forces", (self.n, 2, 4, 3)),
                                     ("info", (self.n, 4)), ("efforts", (self.n, D)))}

    def good(self):
        from thormang_isaacgym_amd import abi
        frames = (abi.tg_contact_frame * 5)()
        for k, f in enumerate(frames):
            f.link = 2 * k + 1
        a = dict(contacts=frames, K=2, extents=(C.c_float * 10)(*([0.1, 0.05] * 5)), mu=0.7, arm=0.1, reg=0.03, rho=0.6,
                 relax=1.6, iters=4, terms=3, dofs=None, num=None)
        a.update({k: C.c_void_p(t.data_ptr()) for k, t in self.out.items()})
        return a

    def call(self, **kw):
        from thormang_isaacgym_amd import _lib
        a = self.good()
        for k, v in kw.items():
            if k == "link":
                a["contacts"][1].link = self.s.L if v == "L" else a["contacts"][0].link if v == "same" else v
            elif k == "ext":
                a["extents"][2] = v
            else:
                a[k] = v
        dofs = [self.s.D] if a["dofs"] == "D" else a["dofs"]
        arr = None if dofs is None else (C.c_int32 * len(dofs))(*dofs)
        num = (0 if dofs is None else len(dofs)) if a["num"] is None else a["num"]
        rc = _lib.lib().tg_contact_qp(self.s.handle, a["contacts"], a["K"], a["extents"], None, None, a["mu"], None,
                                      a["arm"], a["reg"], a["rho"], a["relax"], a["iters"], a["terms"], None, a["tau"],
                                      a["wrench"], a["forces"], a["info"], a["efforts"], arr, num, 0)
        return rc, _lib.lib().tg_last_error().decode()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in self.out.values())


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
    rc, msg = t.call(**change)
    assert rc == -1, msg                                                     # TG_ERR_ARG
    assert msg.startswith("tg_contact_qp: ") and text in msg, msg
    assert t.untouched()


@pytest.mark.gpu
def test_accepted_calls_write_every_element():
    import torch
    t = _shared()
    assert t.untouched()
    own = {k: torch.full_like(o, NAN) for k, o in t.out.items()}
    ptr = {k: C.c_void_p(o.data_ptr()) for k, o in own.items()}
    for keep in ptr:                                                         # each output alone
        rc, msg = t.call(**{k: (v if k == keep else None) for k, v in ptr.items()})
        assert rc == 0, msg
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in own.values()) and t.untouched()
    rc, msg = t.call(K=4, iters=256, **ptr_for(t, 4))                        # the limits of both counts
    assert rc == 0, msg
    torch.cuda.synchronize()


def ptr_for(t, K):
    """NaN-free outputs for K contacts (kept alive on the sim object)."""
    import torch
    D = t.s.D
    t.big = {k: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
             for k, shape in (("tau", (t.n, 6 + D)), ("wrench", (t.n, K, 6)), ("forces", (t.n, K, 4, 3)),
                              ("info", (t.n, 4)), ("efforts", (t.n, D)))}
    return {k: C.c_void_p(v.data_ptr()) for k, v in t.big.items()}
