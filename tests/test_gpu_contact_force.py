"""Net contact force tensor (tg_set_net_contact_force_tensor) on the GPU.

* single rigid bodies: the momentum identity m dv = dt (m g + F), all three
  components, on the plane and on a constant slope (heightfield kernel);
* articulated models: per-link F_z against the fp64 oracle's stored-velocity
  multipliers, with the oracle's own fp32 build as the error yardstick, and
  the structure the solver guarantees (zeros without shapes, F_z >= 0, the
  Coulomb cone, a full rewrite by every simulate);
* nothing else moves: the physics is bit-identical with and without the
  tensor, and the walk task's obs / reward / resets do not depend on it.

Batches are ragged against the workgroup (35 envs: three workgroups of 16, the
whole-body model's 8: five) with a different state per env."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.oracle_lib import lib as oracle_lib, physics_step

pytestmark = pytest.mark.gpu

N = 35
G = 9.81


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


# ------------------------------------------------------------------ small math
def qmul(a, b):
    """Hamilton product, quaternions xyzw."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qaxis(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(ang / 2) * a, [np.cos(ang / 2)]])


def qrot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ------------------------------------------------------------------ single rigid body
THETA = 0.2   # the slope z = tan(THETA) x


def _body_sim(shape, ground, solver, substeps):
    from thormang_isaacgym_amd.sim import Sim
    m = pm.sphere_body(0.1) if shape == "sphere" else pm.box_body()
    mu = {"flat": 0.5, "slope_mu0": 0.0, "slope_mu1": 1.0}[ground]
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=N, dt=0.01, substeps=substeps, solver_type=solver,
                                                ground_friction=mu)
    s = Sim(m, sp, N, "cuda:0")
    assert not s.jit, "the known-answer bodies are compiled in"
    s.env_dirty.fill_(1)
    s.set_shape_friction_indexed(torch.full((N, 1), float(mu), device="cuda:0"), torch.arange(N))
    if ground != "flat":
        h = np.repeat((np.tan(THETA) * np.arange(80) * 0.5)[:, None], 80, 1).astype(np.float32)
        s.set_heightfield(h, 0.5, 1.0, 0.0, 0.0, friction=mu)
    return s, m.links[0].mass, float(sp.dt), mu


def _body_state(rs, case, ground, d):
    """[N,13] start states: the body's lowest point on the surface (``d`` its
    half height / radius), a different place, yaw and velocity per env."""
    root = np.zeros((N, 13), np.float32)
    slope = ground != "flat"
    nrm = np.array([-np.sin(THETA), 0.0, np.cos(THETA)]) if slope else np.array([0.0, 0.0, 1.0])
    qt = qaxis([0, 1, 0], -THETA) if slope else np.array([0.0, 0.0, 0.0, 1.0])   # body z onto the normal
    Rt = qrot(qt)
    for e in range(N):
        x, y = (rs.uniform(10, 30), rs.uniform(5, 35)) if slope else rs.uniform(-2, 2, 2)
        ps = np.array([x, y, np.tan(THETA) * x if slope else 0.0])
        gap = rs.uniform(0.001, 0.01) if case == "land" else 0.0
        root[e, 0:3] = ps + (d + gap) * nrm
        root[e, 3:7] = qmul(qt, qaxis([0, 0, 1], rs.uniform(-np.pi, np.pi)))
        a = rs.uniform(-np.pi, np.pi)
        tang = Rt @ np.array([np.cos(a), np.sin(a), 0.0])
        if case == "land":
            root[e, 7:10] = -rs.uniform(1.0, 2.0) * nrm + 0.2 * tang
        elif case == "slide":
            root[e, 7:10] = 1.0 * tang
        elif case == "spin":
            root[e, 7:10] = 0.3 * tang
            root[e, 10:13] = rs.normal(0, 5.0, 3)
    return root, nrm


@pytest.mark.parametrize("substeps", [1, 2])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("ground", ["flat", "slope_mu0", "slope_mu1"])
def test_single_body_momentum_identity(ground, solver, substeps):
    """kat_box / kat_sphere: the root state's linear velocity is the COM's, so
    m (v_after - v_before) = dt (m g + F) to rounding, per component.  Bound
    (derived, ISSUE): 64 ulp32(max|v|) m / dt + 1e-5 |F| -- the rounding of
    the stored velocity and of the sums.  Resting, landing, sliding (box, 1
    m/s tangential, yawed) and spinning (sphere) starts; then free flight
    reads exactly 0."""
    _cuda()
    rs = np.random.default_rng(7)
    worst = {}
    for shape, d, cases in (("box", 0.05, ("rest", "land", "slide")), ("sphere", 0.1, ("rest", "land", "spin"))):
        s, mass, dt, mu = _body_sim(shape, ground, solver, substeps)
        cf = s.acquire_net_contact_force_tensor()
        assert cf.shape == (N, 1, 3) and cf is s.acquire_net_contact_force_tensor()
        assert s.contact_link_indices == [0]
        for case in cases:
            root, nrm = _body_state(rs, case, ground, d)
            s.root_state.copy_(torch.from_numpy(root))
            s.simulate()
            va = s.root_state.cpu().numpy().astype(np.float64)[:, 7:10]
            F = cf.cpu().numpy().astype(np.float64)[:, 0, :]
            vb = root.astype(np.float64)[:, 7:10]
            assert np.isfinite(F).all() and np.isfinite(va).all()
            lhs = mass * (va - vb) / dt
            rhs = mass * np.array([0.0, 0.0, -G]) + F
            err = np.abs(lhs - rhs).max(axis=1)
            vmax = np.maximum(np.abs(va).max(axis=1), np.abs(vb).max(axis=1))
            bound = np.array([64 * ulp32(v) for v in vmax]) * mass / dt + 1e-5 * np.linalg.norm(F, axis=1)
            worst[(shape, case)] = (float(err.max()), float(bound.min()), float((err / bound).max()))
            print(ground, solver, substeps, shape, case, "max err %.3e N, min bound %.3e N, worst ratio %.3f"
                  % worst[(shape, case)])
            assert (F @ nrm > 0.1 * mass * G).all(), "every env is in contact in this case"
            assert (err <= bound).all(), (shape, case, worst[(shape, case)])
            if case == "rest" and (ground == "flat" or (shape == "box" and ground == "slope_mu1")):
                # at rest it stays at rest: F = -m g up to the residual velocity over dt
                assert np.abs(va).max() < 1e-3
                assert (np.abs(F + mass * np.array([0.0, 0.0, -G])).max(axis=1) <=
                        bound + mass * np.abs(va).max(axis=1) / dt).all()
            if ground == "slope_mu0":   # no friction: the force is along the slope's normal
                Ft = F - np.outer(F @ nrm, nrm)
                assert (np.linalg.norm(Ft, axis=1) <= 1e-5 * np.linalg.norm(F, axis=1)).all()
            if case == "slide":   # one patch: the Coulomb cone, on the plane and on the slope
                Fn = F @ nrm
                Ft = np.linalg.norm(F - np.outer(Fn, nrm), axis=1)
                assert (Ft <= mu * Fn * (1 + 1e-4) + 1e-5 * np.linalg.norm(F, axis=1)).all()
                if ground == "flat":   # 1 m/s cannot be stopped in one step: sliding at the bound
                    assert (Ft >= mu * Fn * (1 - 1e-3)).all()
        # free flight above the contact distance: exactly 0 (and the tensor is rewritten)
        assert float(cf.abs().max()) > 0
        root[:, 2] += 1.0
        s.root_state.copy_(torch.from_numpy(root))
        s.simulate()
        assert float(cf.abs().max()) == 0.0
        s.close()


def test_zero_substeps_write_zeros_and_disable_stops_writing():
    _cuda()
    s, mass, dt, mu = _body_sim("box", "flat", 1, 2)
    cf = s.acquire_net_contact_force_tensor()
    root, _ = _body_state(np.random.default_rng(1), "rest", "flat", 0.05)
    s.root_state.copy_(torch.from_numpy(root))
    s.simulate()
    assert float(cf[:, 0, 2].min()) > 0
    sp = s.get_sim_params()
    sub = sp.substeps
    sp.substeps = 0
    s.set_sim_params(sp)
    s.simulate()
    assert float(cf.abs().max()) == 0.0
    sp.substeps = sub
    s.set_sim_params(sp)
    from thormang_isaacgym_amd._lib import check, lib
    check(lib().tg_set_net_contact_force_tensor(s.handle, None), "disable")
    cf.fill_(-1.0)
    s.simulate()
    assert float(cf.max()) == -1.0
    s.close()


def test_jit_model_is_refused_with_a_message():
    _cuda()
    from thormang_isaacgym_amd._lib import lib
    from thormang_isaacgym_amd.sim import Sim
    m = pm.jit_walker()
    desc, sp, *_ = pm.sim(m, n=4)
    s = Sim(m, sp, 4, "cuda:0")
    assert s.jit
    t = torch.full((4, s.L, 3), 5.0, device="cuda:0")
    rc = lib().tg_set_net_contact_force_tensor(s.handle, C.c_void_p(t.data_ptr()))
    assert rc < 0 and b"compiled-in" in lib().tg_last_error()
    with pytest.raises(RuntimeError):
        s.acquire_net_contact_force_tensor()
    s.close()


# ------------------------------------------------------------------ articulated models
def _lowest_z(m, Rroot, q):
    """Lowest z of the collision shapes with the root origin at 0, orientation Rroot."""
    fk = m.forward_kinematics(q)
    z = np.inf
    for sh in m.shapes:
        R, p = fk[m.link_index(sh.link)]
        Rs = Rroot @ R @ np.asarray(sh.rot)
        c = Rroot @ (p + R @ np.asarray(sh.pos))
        if sh.kind == "box":
            z = min(z, c[2] - sum(abs(Rs[2, k]) * sh.params[k] for k in range(3)))
        elif sh.kind == "sphere":
            z = min(z, c[2] - sh.params[0])
        else:
            z = min(z, c[2] - sh.params[0] * np.sqrt(max(0.0, 1 - Rs[2, 2] ** 2)) - sh.params[1])
    return z


_ART = {}


def _articulated_state(name):
    """Start states (CPU): the task's reset pose with a random yaw and a tilt
    of at most 0.1 rad on the root, lowered until the lowest shape point is
    0 .. 1 mm inside the ground; TGS with the cfg's iterations, no damping."""
    from tests.gpu_harness import NumpyDraws, OracleGogoro, OracleWalk, parity_cfg, walk_cfg
    if name == "gogoro":
        cfg = parity_cfg(N)
        cfg["sim"]["physx"]["solver_type"] = 1
        o = OracleGogoro(cfg, NumpyDraws(3), threads=1)
        props = o.a["dof_props"]
    else:
        cfg = walk_cfg(N, solver_type=1)
        if name == "thormang_wb":
            cfg["env"]["asset"] = dict(cfg["env"].get("asset", {}), wholeBodyCollision=True)
        o = OracleWalk(cfg, NumpyDraws(3), threads=1)
        props = o.props
    m, D = o.model, o.D
    assert m.name == name or name in ("gogoro",), m.name
    o.sp.linear_damping = o.sp.angular_damping = 0.0
    root = o.a["root"].copy()
    dof = o.a["dof_state"].copy()
    pt = o.a["pos_target"].copy()
    vt = o.a["vel_target"].copy() if "vel_target" in o.a else np.zeros((N, D), np.float32)
    rs = np.random.default_rng(11)
    for e in range(N):
        ax = rs.normal(size=2)
        q = qmul(qaxis([0, 0, 1], rs.uniform(-np.pi, np.pi)), qaxis([ax[0], ax[1], 0.0], rs.uniform(0.0, 0.1)))
        root[e, 3:7] = q
        qd = {n: float(dof[e * D + i, 0]) for i, n in enumerate(m.dof_names)}
        root[e, 2] = -_lowest_z(m, qrot(q), qd) - rs.uniform(0.0, 1e-3)
        root[e, 7:13] = rs.normal(0, 0.05, 6)
    return dict(o=o, m=m, D=D, root=root, dof=dof, props=props, pt=pt, vt=vt)


def _articulated(name):
    """The start states (cached, never modified) with a Sim at them after one
    simulate: its live tensor ``cf`` and that simulate's forces ``F``."""
    if name in _ART:
        return _ART[name]
    from thormang_isaacgym_amd.sim import Sim
    a = _articulated_state(name)
    o, m, root, dof, props, pt, vt = (a[k] for k in ("o", "m", "root", "dof", "props", "pt", "vt"))
    s = Sim(m, o.sp, N, "cuda:0")
    assert not s.jit
    s.root_state.copy_(torch.from_numpy(root))
    s.dof_state.copy_(torch.from_numpy(dof))
    s.dof_props.copy_(torch.from_numpy(props))
    s.dof_pos_target.copy_(torch.from_numpy(pt))
    s.dof_vel_target.copy_(torch.from_numpy(vt))
    s.env_dirty.fill_(1)
    cf = s.acquire_net_contact_force_tensor()
    s.simulate()
    a.update(sim=s, cf=cf, F=cf.cpu().numpy().astype(np.float64))
    _ART[name] = a
    return a


def _row_layout(m):
    """(link of row i or -1 for a friction row) in the solver's static row
    order: per shape its normal rows (4 box corners, else 1), then 2 or 3 friction rows."""
    out = []
    for sh in m.shapes:
        nr = 4 if sh.kind == "box" else 1
        out += [m.link_index(sh.link)] * nr + [-1] * (2 if nr == 1 else 3)
    return out


def _oracle_fz(a, e, precision):
    """Env e's per-link F_z from the oracle's stored-velocity multipliers: the
    normal rows' sum / h, averaged over the substeps (flat ground: the normal
    is e_z and the friction rows are horizontal).  One single-threaded oracle
    call per substep index, each from the same start state."""
    L = oracle_lib(precision)
    L.oracle_dump_set.argtypes = [C.c_int, C.c_int]
    L.oracle_dump_read.argtypes = [C.c_void_p, C.c_int]
    o, m, D = a["o"], a["m"], a["D"]
    S, h = int(o.sp.substeps), float(o.sp.dt) / int(o.sp.substeps)
    layout = _row_layout(m)
    fz = np.zeros(m.num_bodies)
    for sub in range(S):
        r = a["root"][e:e + 1].copy()
        d = a["dof"][e * D:(e + 1) * D].copy()
        L.oracle_dump_set(0, sub)
        try:
            physics_step(o.desc, o.sp, r, d, np.ascontiguousarray(a["props"][:, e:e + 1, :]), a["pt"][e:e + 1].copy(),
                         a["vt"][e:e + 1].copy(), threads=1, L=L)
            buf = np.zeros(4096)
            L.oracle_dump_read(buf.ctypes.data, 4096)
        finally:
            L.oracle_dump_set(-1, 0)
        K = int(buf[0])
        assert K == len(layout), (K, len(layout))
        phi = buf[2100 + 8 * np.arange(K) + 6]
        # the normal / friction split is unambiguous: every normal row's separation is off 0
        assert all((abs(phi[i]) > 1e-6) == (layout[i] >= 0) for i in range(K)), phi
        for i in range(K):
            if layout[i] >= 0:
                fz[layout[i]] += buf[2500 + i] / h / S
    return fz


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_articulated_fz_matches_the_fp64_oracle(name):
    """Per-link F_z against the fp64 oracle; the yardstick is the oracle's own
    fp32 build on the same quantity: the GPU's largest error must stay within
    4x the control's largest + 1e-6 M |g| (DESIGN 2.3 records up to 2.7x on
    qdd for the kernel's other summation orders).  Both maxima are taken over
    all 35 envs: the control's error spreads over a factor of 30 between envs
    (a normal row's multiplier is its separation's rounding times m_eff / h^2,
    and the envs differ in which corners bear), so the maximum over a handful
    is mostly the draw -- over envs 0, 7, 16, 23, 34 the control reads 2.8e-3
    N on thormang, over all 35 it reads 6.8e-3 N.  The handful's figures are
    printed beside the full ones.  Measured on the MI355X,
    GPU / control: thormang 1.17e-2 / 6.8e-3 N over all envs (ratio 1.71; the
    five envs alone 1.17e-2 / 2.8e-3 N, 4.24), gogoro 3.6e-4 / 2.8e-4 N (1.31)."""
    _cuda()
    a = _articulated(name)
    m = a["m"]
    M = sum(l.mass for l in m.links)
    e_gpu, e_ctl = np.zeros(N), np.zeros(N)
    for e in range(N):
        f64 = _oracle_fz(a, e, "f64")
        f32 = _oracle_fz(a, e, "f32")
        assert f64.max() > 0.05 * M * G, "the env carries weight on the ground"
        e_gpu[e] = np.abs(a["F"][e, :, 2] - f64).max()
        e_ctl[e] = np.abs(f32 - f64).max()
    few = [0, 7, 16, 23, 34]
    for what, g, c in (("envs 0,7,16,23,34", e_gpu[few].max(), e_ctl[few].max()), ("all envs", e_gpu.max(), e_ctl.max()),
                       ("median env", np.median(e_gpu), np.median(e_ctl))):
        print(name, "F_z error vs fp64 oracle, %s: GPU %.4e N, fp32 oracle (control) %.4e N, ratio %.2f, M|g| %.1f N"
              % (what, g, c, g / max(c, 1e-30), M * G))
    assert e_gpu.max() <= 4 * e_ctl.max() + 1e-6 * M * G, (e_gpu.max(), e_ctl.max())


@pytest.mark.parametrize("name", ["thormang", "gogoro", "thormang_wb"])
def test_articulated_structure(name):
    """What the solver guarantees, no measured tolerance: links without shapes
    read exactly 0, F_z >= 0, the Coulomb cone per one-patch link, and a full
    rewrite: lifted out of contact, the next simulate writes zeros."""
    _cuda()
    a = _articulated(name)
    m, F, s = a["m"], a["F"], a["sim"]
    assert np.isfinite(F).all()
    links = s.contact_link_indices
    rest = [l for l in range(m.num_bodies) if l not in links]
    assert (F[:, rest, :] == 0).all()
    assert (F[:, :, 2] >= 0).all()
    assert (F[:, links, 2].sum(axis=1) > 0).all(), "every env touches the ground"
    # envs differ (a wrong env / lane index would repeat or shift rows)
    assert len({tuple(np.round(F[e, links].ravel(), 3)) for e in range(N)}) == N
    mu_g = float(a["o"].sp.ground_friction)
    for sh in m.shapes:   # every link here carries one shape, hence one patch
        l = m.link_index(sh.link)
        mu = 0.5 * (float(sh.friction) + mu_g)
        assert (np.linalg.norm(F[:, l, :2], axis=1) <= mu * F[:, l, 2] * (1 + 1e-4) + 1e-30).all(), sh.link
    # lift out of contact with a root write: zeros on the next simulate
    keep = s.root_state.clone()
    keepd = s.dof_state.clone()
    up = s.root_state.clone()
    up[:, 2] += 2.0
    s.set_actor_root_state_indexed(up, s.all_ids)
    s.simulate()
    assert float(a["cf"].abs().max()) == 0.0
    s.root_state.copy_(keep)
    s.dof_state.copy_(keepd)


def test_wholebody_kneel_loads_shins_and_hands():
    """thormang_wb (the SWXON layout: more contact rows than groups) in the
    kneel pose of the whole-body tests: after the fall the shins and the hands
    carry force, the structure holds, and the links' F_z sum to the weight."""
    _cuda()
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_kneel_cfg
    cfg = walk_kneel_cfg(N)
    cfg["env"]["enableContactForces"] = True
    env = make_gpu_walk(cfg, NumpyDraws(0))
    m = env.model
    assert m.name == "thormang_wb" and len(m.shapes) == 6
    acc = torch.zeros(N, m.num_bodies, 3, device="cuda:0")
    act = torch.zeros(N, m.num_dof, device="cuda:0")
    for t in range(150):   # (zero actions: down and at rest after ~100 steps, tests/test_walk_wholebody.py)
        env.step(act)
        if t >= 100:
            acc += env.contact_forces
    F = (acc / 50).cpu().numpy().astype(np.float64)
    last = env.contact_forces.cpu().numpy()
    links = env.sim.contact_link_indices
    assert np.isfinite(last).all() and (last[:, :, 2] >= 0).all()
    assert (last[:, [l for l in range(m.num_bodies) if l not in links]] == 0).all()
    names = {m.links[l].name: l for l in links}
    shins = [names["l_leg_kn_p_link"], names["r_leg_kn_p_link"]]
    hands = [names["l_arm_wr_p_link"], names["r_arm_wr_p_link"]]
    M = sum(l.mass for l in m.links)
    print("kneel: mean F_z shins", F[:, shins, 2].mean(), "hands", F[:, hands, 2].mean(), "total/weight",
          F[:, :, 2].sum(axis=1).mean() / (M * G))
    assert (F[:, shins, 2].sum(axis=1) > 0.05 * M * G).all()
    assert (F[:, hands, 2].sum(axis=1) > 0).all()
    # it lies still by then: the mean vertical force over 50 steps carries the weight
    assert np.abs(F[:, :, 2].sum(axis=1) / (M * G) - 1).max() < 0.1


# ------------------------------------------------------------------ nothing else moved
@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_physics_is_bit_identical_with_and_without_the_tensor(name):
    _cuda()
    from thormang_isaacgym_amd.sim import Sim
    a = _articulated(name)

    def run(acquire):
        s = Sim(a["m"], a["o"].sp, N, "cuda:0")
        s.root_state.copy_(torch.from_numpy(a["root"]))
        s.dof_state.copy_(torch.from_numpy(a["dof"]))
        s.dof_props.copy_(torch.from_numpy(a["props"]))
        s.dof_pos_target.copy_(torch.from_numpy(a["pt"]))
        s.dof_vel_target.copy_(torch.from_numpy(a["vt"]))
        s.env_dirty.fill_(1)
        cf = s.acquire_net_contact_force_tensor() if acquire else None
        for _ in range(50):
            s.simulate()
        out = s.root_state.cpu().numpy().copy(), s.dof_state.cpu().numpy().copy()
        assert cf is None or float(cf.abs().max()) > 0
        s.close()
        return out

    (r0, d0), (r1, d1) = run(False), run(True)
    assert np.isfinite(r0).all()
    assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32))
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


def test_walk_task_exposes_feet_forces_and_is_otherwise_unchanged():
    """ThormangWalk with env.enableContactForces against one without, same
    seed, 50 steps: resets, time-outs and progress identical; obs and reward
    within the fused-vs-separate difference the project records for the walk
    (the enabled task runs the separate post-physics launch:
    tests/test_gpu_walk.py test_gpu_walk_fused_step_equals_separate_calls,
    1e-5 per step, teacher-forced -- the two step kernels are separately
    optimised fast-math code); as there, the enabled env is re-synced from
    the other before every step.  The extras carry the tensor's foot rows."""
    _cuda()
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_cfg
    envs = []
    for on in (False, True):
        cfg = walk_cfg(N)
        if on:
            cfg["env"]["enableContactForces"] = True
        envs.append(make_gpu_walk(cfg, NumpyDraws(5)))
    off, on = envs
    assert off.contact_forces is None and "feet_contact_force" not in off.extras
    assert on.contact_forces.shape == (N, on.model.num_bodies, 3)
    assert [on.model.links[int(i)].name for i in on.feet_indices] == ["l_leg_foot_link", "r_leg_foot_link"]
    rs = np.random.default_rng(9)
    dobs = drew = 0.0
    seen = 0.0
    for _ in range(50):
        for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "actions", "last_actions", "commands"):
            getattr(on, name).copy_(getattr(off, name))
        on.sim.root_state.copy_(off.sim.root_state)
        on.sim.dof_state.copy_(off.sim.dof_state)
        if off.push_enabled:
            on.sim.body_force.copy_(off.sim.body_force)
        act = torch.from_numpy(rs.uniform(-0.5, 0.5, (N, on.model.num_dof)).astype(np.float32)).cuda()
        o0, r0, z0, x0 = off.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        assert torch.equal(z0, z1) and torch.equal(x0["time_outs"], x1["time_outs"])
        assert torch.equal(off.progress_buf, on.progress_buf)
        dobs = max(dobs, float((o0["obs"] - o1["obs"]).abs().max()))
        drew = max(drew, float((r0 - r1).abs().max()))
        ff = x1["feet_contact_force"]
        assert ff.shape == (N, 2, 3) and torch.equal(ff, on.contact_forces[:, on.feet_indices])
        seen = max(seen, float(ff[:, :, 2].max()))
    print("walk with / without the tensor: max |d obs| %.3e, max |d reward| %.3e" % (dobs, drew))
    assert seen > 0
    assert dobs <= 1e-5 and drew <= 1e-5, (dobs, drew)
