"""The float64 reference of the contact force distribution (tests/contact_qp_ref.py)
pinned on its own, without the GPU, and the scenarios tests/test_gpu_contact_qp.py
shares: Thormang at the ThormangWalk default stance (2 envs, env 1 with one arm
joint offset) on both soles (walk_sole_patch: 0.22 x 0.15 m, the CoM 0.81 m
above them, 43.7 kg) under eight load cases.

(1) interior case: the wrenches agree with contact_id_ref at equal shares within
    the effect of reg; (2) KKT: feasible, and no feasible perturbation lowers the
    objective; (3) the infeasible cases end on the sole's edge and on the cone;
(4) a zero share removes its contact exactly; (5) the convergence table behind
the defaults, asserted (profiles/r13/contact_qp_convergence.txt is its print)."""
import functools

import numpy as np
import pytest

from tests.contact_id_ref import contact_id_ref
from tests.contact_qp_ref import (DEFAULTS, Problem, contact_qp_converged, contact_qp_ref, patch_vertices,
                                  project_cone)
from tests.id_ref import Kinematics
from tests.test_contact_id_reference import closed_loop_case
from thormang_isaacgym_amd.sim import load_model

MU = 0.7
TABLE_ITERS = (16, 32, 64, 128)
TABLE_BOUND = 1e-2   # of the largest force, at the default iters, on every load case


@functools.lru_cache(maxsize=None)
def stance():
    """(m, root, dof, contacts, extents, kin) of the standing Thormang on both soles, read-only."""
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_patch
    m = load_model("thormang")
    desc, _sp, root, dof, *_ = closed_loop_case(m)
    patches = [walk_sole_patch(m, l) for l in walk_feet_indices(m)]
    con = [(int(l), tuple(p[0])) for l, p in zip(walk_feet_indices(m), patches)]
    ext = [p[1] for p in patches]
    for x in (root, dof):
        x.setflags(write=False)
    return m, root, dof, con, ext, Kinematics(m, root, dof, desc)


def load_cases(n, D, K, seed=1):
    """name -> keyword arguments of the reference (and, as tensors, of Sim.contact_qp): the load cases of the
    convergence trial, made by ``accel`` and by tilted ``normals``."""
    def acc(ax=0.0, ay=0.0):
        a = np.zeros((n, 6 + D), np.float32)
        a[:, 0], a[:, 1] = ax, ay
        return a

    tilt = np.zeros((n, K, 3), np.float32)
    tilt[...] = (0.35, -0.2, 1.0)
    rs = np.random.default_rng(seed)
    return {
        "stand": dict(mu=MU),
        "slope": dict(mu=0.3, normals=tilt),                                  # friction binds on the tilted ground
        "share": dict(mu=MU, share=np.tile(np.float32([1.0, 0.3][:K] + [1.0] * (K - 2)), (n, 1))),
        "toe": dict(mu=MU, accel=acc(-1.2)),                                  # braking: the centre of pressure near the toes
        "beyond": dict(mu=MU, accel=acc(-3.0)),                               # ... and beyond them: infeasible
        "lateral": dict(mu=0.2, accel=acc(0.0, 3.0)),                         # wants 0.31 of the load sideways at mu 0.2
        "frictionless": dict(mu=0.0, accel=acc(0.5, 0.5)),
        "general": dict(mu=MU, accel=rs.normal(0, 1.0, (n, 6 + D)).astype(np.float32)),
    }


@functools.lru_cache(maxsize=None)
def converged(name):
    m, root, dof, con, ext, kin = stance()
    pr = []
    out = contact_qp_converged(m, root, dof, con, ext, kin=kin, velocity=False, problems=pr,
                               **load_cases(kin.n, kin.D, len(con))[name])
    out["problems"] = pr
    return out


def test_interior_case_agrees_with_the_least_squares_distribution():
    """(1) standing, flat, mu 0.7: every vertex force is strictly inside its cone, so the cones do nothing and the
    call differs from tg_contact_inverse_dynamics (equal shares) only by reg.  At the minimiser G_kv^T W d = reg
    f_kv for the balance error d = b[0:6] - sum G f (checked vertex by vertex), so the error is reg times the largest
    vertex force.  The bound on the wrenches is therefore reg f_max / F, F the total force: on the forces relative to
    F, on the moments relative to F r_max, r_max the longest lever arm of a vertex about the root's com, about which
    the balance is formed.  At this symmetric stance nothing else tells the two distributions apart (each foot's
    moment about its centre is the one the com's 11 mm offset asks for).  Measured 3.6e-3 and 3.7e-3 against
    4.7e-3; the base rows themselves (printed) are 8e-3 of F, through the moment error's lever arm."""
    m, root, dof, con, ext, kin = stance()
    c = converged("stand")
    reg = DEFAULTS["reg"]
    _tau, lam = contact_id_ref(m, root, dof, con, kin=kin, velocity=False)
    _p, pv = patch_vertices(kin, con, ext)
    for e in range(kin.n):
        pr = c["problems"][e]
        f = c["forces"][e].reshape(-1, 3)
        fn = (f * pr.nrm).sum(-1)
        ft = np.linalg.norm(f - fn[:, None] * pr.nrm, axis=-1)
        assert (fn > 0).all() and (ft < 0.5 * pr.mu * fn).all()                # strictly inside
        fmax, F = np.linalg.norm(f, axis=-1).max(), np.linalg.norm(c["b"][e, :3])
        rmax = np.linalg.norm(pv[e] - kin.c[e, 0], axis=-1).max()
        d = c["tau"][e, :6]
        for j in range(len(f)):                                               # stationarity, vertex by vertex
            r = pv[e].reshape(-1, 3)[j] - kin.c[e, 0]
            g = d[:3] + np.cross(d[3:] / 0.1 ** 2, r)
            # (1e-6: tau's base rows come through the oracle's float32 Jacobian columns, good to 1.2e-7 m)
            assert np.abs(g - reg * f[j]).max() <= 1e-6 * fmax
        bound = reg * fmax / F
        fig = {"env": e, "bound": bound, "base_force_rel": np.linalg.norm(d[:3]) / F,
               "wrench_force_rel": np.abs(c["wrench"][e, :, :3] - lam[e, :, :3]).max() / F,
               "wrench_moment_rel": np.abs(c["wrench"][e, :, 3:] - lam[e, :, 3:]).max() / (F * rmax)}
        print(fig)
        assert fig["wrench_force_rel"] <= bound and fig["wrench_moment_rel"] <= bound


@pytest.mark.parametrize("name", ["stand", "slope", "share", "toe", "beyond", "lateral", "frictionless", "general"])
def test_kkt_at_the_converged_point(name):
    """(2) every force is in its cone, and the objective does not fall under 1000 random feasible perturbations
    (the point plus noise of 1e-4 .. 10 N per component, projected back on the cones)."""
    c = converged(name)
    rs = np.random.default_rng(5)
    for e, pr in enumerate(c["problems"]):
        f = np.concatenate([c["forces"][e, i] for i in pr.on])
        assert pr.feasible(f, tol=1e-12 * np.abs(f).max())
        base = pr.objective(f)
        worst = 0.0
        for t in range(1000):
            g = project_cone(f + rs.normal(0, 10.0 ** rs.uniform(-4, 1), f.shape), pr.nrm, pr.mu)
            worst = min(worst, pr.objective(g) - base)
        print({"case": name, "env": e, "objective": base, "lowest_change": worst})
        assert worst >= -1e-9 * max(base, 1.0)


def _cop(forces, nrm, ext):
    """The centre of pressure of each contact in patch coordinates (x, y) from the vertex normal forces."""
    sx = np.array([1.0, 1.0, -1.0, -1.0])
    sy = np.array([1.0, -1.0, -1.0, 1.0])
    out = []
    for i, (hx, hy) in enumerate(ext):
        fn = (forces[i] * nrm[4 * i:4 * i + 4]).sum(-1)
        out.append(((fn * sx * hx).sum() / fn.sum(), (fn * sy * hy).sum() / fn.sum()))
    return np.array(out)


def test_infeasible_cases_end_on_the_edge_and_on_the_cone():
    """(3) the com beyond the toes: tau[0:6] is non-zero and each sole's centre of pressure lies on its front edge;
    a lateral demand of 0.31 of the load at mu 0.2: tau[0:6] is non-zero and every loaded vertex has |f_t| = mu f_n;
    both to 1e-9 (of the half extent, of the largest force)."""
    _m, _root, _dof, _con, ext, _kin = stance()
    c = converged("beyond")
    for e, pr in enumerate(c["problems"]):
        cop = _cop(c["forces"][e], pr.nrm, ext)
        print({"case": "beyond", "env": e, "cop": cop.tolist(), "base": c["tau"][e, :6].tolist()})
        assert np.linalg.norm(c["tau"][e, :3]) > 10.0
        assert np.abs(cop[:, 0] - [x[0] for x in ext]).max() <= 1e-9 * ext[0][0]
    c = converged("lateral")
    for e, pr in enumerate(c["problems"]):
        f = c["forces"][e].reshape(-1, 3)
        fn = (f * pr.nrm).sum(-1)
        ft = np.linalg.norm(f - fn[:, None] * pr.nrm, axis=-1)
        fmax = np.abs(f).max()
        loaded = fn > 1e-6 * fmax
        print({"case": "lateral", "env": e, "f_n": fn.tolist(), "ratio": (ft[loaded] / fn[loaded]).tolist(),
               "base": c["tau"][e, :6].tolist()})
        assert np.linalg.norm(c["tau"][e, :3]) > 10.0 and loaded.sum() >= 4
        assert np.abs(ft[loaded] - 0.2 * fn[loaded]).max() <= 1e-9 * fmax


def test_zero_share_removes_the_contact():
    """(4) s_k = 0: the contact's forces and wrench are exactly 0.0 and every other output equals that of the call
    without it; every share 0: tau = b, no forces."""
    m, root, dof, con, ext, kin = stance()
    kw = dict(kin=kin, velocity=False, mu=MU)
    share = np.array([[0.0, 1.0], [0.7, 0.0]])
    got = contact_qp_ref(m, root, dof, con, ext, share=share, **kw)
    for e, keep in ((0, 1), (1, 0)):
        one = contact_qp_ref(m, root, dof, [con[keep]], [ext[keep]], share=share[:, [keep]], **kw)
        assert (got["forces"][e, 1 - keep] == 0.0).all() and (got["wrench"][e, 1 - keep] == 0.0).all()
        assert np.array_equal(got["forces"][e, keep], one["forces"][e, 0])
        assert np.array_equal(got["wrench"][e, keep], one["wrench"][e, 0])
        assert np.array_equal(got["tau"][e], one["tau"][e]) and np.array_equal(got["info"][e], one["info"][e])
        assert np.abs(got["forces"][e, keep]).max() > 10.0
    none = contact_qp_ref(m, root, dof, con, ext, share=np.zeros((2, 2)), **kw)
    assert (none["forces"] == 0.0).all() and (none["wrench"] == 0.0).all() and np.array_equal(none["tau"], none["b"])
    assert (none["info"][:, 2:] == 0.0).all()
    negative = contact_qp_ref(m, root, dof, con, ext, share=np.array([[-1.0, 1.0], [0.7, np.nan]]), **kw)
    assert np.array_equal(negative["forces"], got["forces"])


def convergence_table():
    """rows (case, largest force, {iters: distance to the converged forces / largest force}, |tau[0:3]| converged)."""
    m, root, dof, con, ext, kin = stance()
    rows = []
    for name, kw in load_cases(kin.n, kin.D, len(con)).items():
        c = converged(name)
        scale = float(np.abs(c["forces"]).max())
        dist = {}
        for it in TABLE_ITERS:
            r = contact_qp_ref(m, root, dof, con, ext, kin=kin, velocity=False, iters=it, **kw)
            dist[it] = float(np.abs(r["forces"] - c["forces"]).max()) / scale
        rows.append((name, scale, dist, float(c["info"][:, 0].max())))
    return rows


def format_table(rows):
    head = f"{'case':<14}{'f_max [N]':>10}" + "".join(f"{'it ' + str(i):>10}" for i in TABLE_ITERS) + f"{'|tau[0:3]| [N]':>16}"
    return "\n".join([head] + [f"{n:<14}{s:>10.1f}" + "".join(f"{d[i]:>10.1e}" for i in TABLE_ITERS) + f"{t:>16.2f}"
                               for n, s, d, t in rows])


def test_convergence_table_behind_the_defaults():
    """(5) the distance of the forces after 16 .. 128 iterations to the converged ones, over the largest force, per
    load case at the defaults (reg 0.03, rho 0.6, relax 1.6): at the default 64 iterations at most 1e-2 everywhere.
    Measured: 4.5e-13 (stand) .. 2.8e-3 (lateral) at 64; 2.9e-7 .. 4.2e-2 at 32."""
    assert DEFAULTS == dict(reg=0.03, rho=0.6, relax=1.6, iters=64) and DEFAULTS["iters"] in TABLE_ITERS
    from thormang_isaacgym_amd import abi
    assert abi.TG_QP_DEFAULTS == DEFAULTS
    rows = convergence_table()
    print(format_table(rows))
    for name, _scale, dist, _t in rows:
        assert dist[DEFAULTS["iters"]] <= TABLE_BOUND, (name, dist)
        assert dist[128] <= dist[16]
