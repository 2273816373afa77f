"""The float64 reference of the inverse dynamics (tests/id_ref.py) is pinned
before the kernel is held to it (tests/test_gpu_id.py): its gravity part is the
plain sum of link weights through the Jacobian, its acceleration part is H a,
its velocity-product accelerations are the derivatives of the oracle's link
velocities, its velocity part satisfies the energy identity of the mass
matrix, and in closed loop with the fp64 oracle's physics step it holds a
posture under gravity and lets moving joints coast.  No GPU needed.

Tolerances.  (a) and (b) are float64 identities of the same arrays: 1e-12
relative.  (c) and (d) compare against central differences of float32 oracle
output at step 1e-3 along the motion; the agreement was measured (figures in
the tests' docstrings) and 4 x the measured value is asserted, as in
tests/test_ik_reference.py."""
import functools

import numpy as np
import pytest

from tests import physics_models as pm
from tests.id_ref import GRAVITY, Kinematics, generalised_velocity, id_ref
from tests.jacobian_ref import mass_matrix_ref
from tests.oracle_lib import physics_step, rigid_body_states
from tests.test_rigid_body_states import advance, random_state
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.sim import load_model

FAR = (300.0, -200.0, 1.0)
N = 3
FD_STEP = 1e-3
# measured worst agreement (relative to the largest reference value) of the central differences, per model
FD_MEASURED = {"thormang": {"ab": 1.2e-5, "alb": 1.2e-5, "energy": 8.7e-6},
               "gogoro": {"ab": 1.7e-5, "alb": 2.2e-5, "energy": 2.4e-4}}


def _case(name, seed=11, n=N):
    m = load_model(name)
    rs = np.random.default_rng(seed)
    root, dof = random_state(m, n, rs)
    ms = rs.uniform(0.8, 1.2, (n, m.num_bodies)).astype(np.float32)
    arm = rs.uniform(0.005, 0.02, (n, m.num_dof)).astype(np.float32)
    return m, root, dof, ms, arm, rs


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_gravity_only_is_the_sum_of_link_weights(name):
    """(a) tau(gravity only) = -sum_l s_l m_l Jv_l^T g, to 1e-12."""
    m, root, dof, ms, arm, rs = _case(name)
    k = Kinematics(m, root, dof)
    g = np.array([0.3, -0.2, -9.81])
    tau = id_ref(m, root, dof, gravity=True, velocity=False, g=g, mass_scale=ms, kin=k)
    want = np.zeros_like(tau)
    for e in range(N):
        for l in range(m.num_bodies):
            want[e] -= ms[e, l].astype(np.float64) * k.li[l, 0] * (k.J[e, l, :3].T @ g)
    assert np.abs(tau - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(want[:, 6:]).max() > 1.0
    # the net force is the total weight, whatever the pose
    total = (ms.astype(np.float64) * k.li[None, :, 0]).sum(axis=1)
    np.testing.assert_allclose(tau[:, :3], -total[:, None] * g[None, :], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_acceleration_enters_through_the_mass_matrix(name):
    """(b) tau(a) - tau(0) = H a, armature included, to 1e-12."""
    m, root, dof, ms, arm, rs = _case(name)
    k = Kinematics(m, root, dof)
    a = rs.normal(0, 2.0, (N, 6 + m.num_dof))
    t0 = id_ref(m, root, dof, mass_scale=ms, armature=arm, kin=k)
    t1 = id_ref(m, root, dof, accel=a, mass_scale=ms, armature=arm, kin=k)
    H = mass_matrix_ref(m, k.root0, dof, mass_scale=ms, armature=arm, J=k.J)
    want = np.einsum("eij,ej->ei", H, a)
    assert np.abs((t1 - t0) - want).max() <= 1e-12 * np.abs(want).max()
    # and alone, with no terms
    t2 = id_ref(m, root, dof, accel=a, gravity=False, velocity=False, mass_scale=ms, armature=arm, kin=k)
    assert np.abs(t2 - want).max() <= 1e-12 * np.abs(want).max()
    no_arm = id_ref(m, root, dof, accel=a, gravity=False, velocity=False, mass_scale=ms, kin=k)
    assert np.abs(no_arm - t2).max() > 1e-3


def _link_velocities(m, desc, root, dof, u_root, qd):
    """The oracle's link com and angular velocities [N, L, 6] at the pose (root, dof) with u held at (u_root, qd)."""
    n, D = root.shape[0], m.num_dof
    r = np.array(root, np.float32)
    r[:, 7:13] = u_root
    d = np.array(dof, np.float32).reshape(n, D, 2).copy()
    d[:, :, 1] = qd
    return rigid_body_states(desc, r, np.ascontiguousarray(d.reshape(n * D, 2)))[..., 7:13].astype(np.float64)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_velocity_product_accelerations_are_derivatives_of_the_link_velocities(name):
    """(c) ab_l and alb_l against central differences of the oracle's link
    velocities along q +- eps qd (root pose moved along u(0:6)) with u held
    fixed, eps = 1e-3.  Measured max |difference| / max |reference|: see
    FD_MEASURED; asserted at 4 x."""
    m, root, dof, ms, arm, rs = _case(name)
    root[:, :3] = 0.0
    desc = abi.ModelDesc(m)
    _tau, ab, alb, _w, _H = id_ref(m, root, dof, desc=desc, parts=True)
    qd = dof.reshape(N, m.num_dof, 2)[:, :, 1]
    rp, dp = advance(m, root, dof, FD_STEP)
    rm, dm = advance(m, root, dof, -FD_STEP)
    vp = _link_velocities(m, desc, rp, dp, root[:, 7:13], qd)
    vm = _link_velocities(m, desc, rm, dm, root[:, 7:13], qd)
    fd = (vp - vm) / (2 * FD_STEP)
    fig = {"model": name, "ab": float(np.abs(fd[..., :3] - ab).max() / np.abs(ab).max()),
           "alb": float(np.abs(fd[..., 3:] - alb).max() / np.abs(alb).max()),
           "max_ab": float(np.abs(ab).max()), "max_alb": float(np.abs(alb).max())}
    print(fig)
    assert fig["max_ab"] > 1.0 and fig["max_alb"] > 1.0
    assert fig["ab"] <= 4 * FD_MEASURED[name]["ab"], fig
    assert fig["alb"] <= 4 * FD_MEASURED[name]["alb"], fig


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_energy_identity(name):
    """(d) u^T h_vel = 0.5 u^T H' u, H' the central difference of
    mass_matrix_ref along the motion (no armature: it is constant).  Both
    sides are the rate of change of the kinetic energy at u' = 0.  Measured
    |difference| / max |0.5 u^T H' u|: see FD_MEASURED; asserted at 4 x."""
    m, root, dof, ms, arm, rs = _case(name)
    root[:, :3] = 0.0
    desc = abi.ModelDesc(m)
    u = generalised_velocity(m, root, dof)
    h = id_ref(m, root, dof, gravity=False, velocity=True, mass_scale=ms, desc=desc)
    rp, dp = advance(m, root, dof, FD_STEP)
    rm, dm = advance(m, root, dof, -FD_STEP)
    Hp = mass_matrix_ref(m, rp.astype(np.float32), dp.astype(np.float32), mass_scale=ms, desc=desc)
    Hm = mass_matrix_ref(m, rm.astype(np.float32), dm.astype(np.float32), mass_scale=ms, desc=desc)
    Hd = (Hp - Hm) / (2 * FD_STEP)
    lhs = np.einsum("ei,ei->e", u, h)
    rhs = 0.5 * np.einsum("ei,eij,ej->e", u, Hd, u)
    fig = {"model": name, "energy": float(np.abs(lhs - rhs).max() / np.abs(rhs).max()), "lhs": lhs.tolist(),
           "rhs": rhs.tolist()}
    print(fig)
    assert np.abs(rhs).max() > 1.0
    assert fig["energy"] <= 4 * FD_MEASURED[name]["energy"], fig


def test_result_does_not_depend_on_the_env_position():
    m, root, dof, ms, arm, rs = _case("thormang", n=2)
    root[1], ms[1] = root[0], ms[0]
    dof.reshape(2, m.num_dof, 2)[1] = dof.reshape(2, m.num_dof, 2)[0]
    root[1, :3] = FAR
    tau = id_ref(m, root, dof, mass_scale=ms)
    assert np.array_equal(tau[0], tau[1]) and np.abs(tau[0]).max() > 1.0


# ---------------------------------------------------------------- closed loop with the fp64 oracle step
CLOSED_LOOP_STEPS, CLOSED_LOOP_N = 60, 2
ARM_SPEED = 0.5          # rad/s, the coasting case's initial arm joint speeds are U(-ARM_SPEED, ARM_SPEED)
HOLD_BOUND = 1e-3        # the project's parity bar, rad
COAST_BOUND = 1e-3       # the same bar on the joint velocities, rad/s


def closed_loop_case(m, seed=5, n=CLOSED_LOOP_N, coasting=False):
    """The fixed-base Thormang at z = 2 under gravity, dt 1/120 x 1 substep,
    every DOF in EFFORT mode with zero gains and an effort limit of 1e4,
    armature 0.01, at rest at lower + U(0.3, 0.7) (upper - lower); with
    ``coasting`` the arm joints start at U(-ARM_SPEED, ARM_SPEED) rad/s.
    Returns (desc, sp, root, dof, props, pt, vt)."""
    rs = np.random.default_rng(seed)
    D = m.num_dof
    st = pm.sim(m, n=n, dt=1.0 / 120.0, substeps=1, gravity=GRAVITY, fix_base_link=True)
    desc, sp, root, dof, props, pt, vt = st
    root[:, 2] = 2.0
    lo, hi = props[abi.TG_PROP_LOWER].astype(np.float64), props[abi.TG_PROP_UPPER].astype(np.float64)
    q0 = (lo + rs.uniform(0.3, 0.7, (n, D)) * (hi - lo)).astype(np.float32)
    dof.reshape(n, D, 2)[:, :, 0] = q0
    props[abi.TG_PROP_ARMATURE] = 0.01
    props[abi.TG_PROP_DRIVE_MODE] = 3
    props[abi.TG_PROP_STIFFNESS] = 0.0
    props[abi.TG_PROP_DAMPING] = 0.0
    props[abi.TG_PROP_EFFORT] = 1e4
    if coasting:
        arms = [d for d, nm in enumerate(m.dof_names) if "_arm_" in nm]
        assert len(arms) >= 12
        dof.reshape(n, D, 2)[:, arms, 1] = rs.uniform(-ARM_SPEED, ARM_SPEED, (n, len(arms))).astype(np.float32)
    return st


@functools.lru_cache(maxsize=None)
def reference_loop(mode):
    """The oracle loop's final (dof [N * D, 2] float32, the initial state):
    mode 'hold' (efforts = tau_ref[6:] each step, at rest), 'free' (zero
    efforts, at rest), 'coast' (both terms, the arms moving), 'coast_gravity'
    (the gravity term alone, the arms moving)."""
    m = load_model("thormang")
    n, D = CLOSED_LOOP_N, m.num_dof
    desc, sp, root, dof, props, pt, vt = closed_loop_case(m, coasting=mode.startswith("coast"))
    dof0 = dof.copy()
    for _ in range(CLOSED_LOOP_STEPS):
        act = np.zeros((n, D), np.float32)
        if mode != "free":
            tau = id_ref(m, root, dof, gravity=True, velocity=mode != "coast_gravity", desc=desc)
            act[:] = tau[:, 6:]
        physics_step(desc, sp, root, dof, props, pt, vt, act=act)
    dof.setflags(write=False)
    dof0.setflags(write=False)
    return dof, dof0


def test_closed_loop_holds_a_posture_under_gravity():
    """(e) 60 steps of efforts = tau_ref[6:] hold the random posture to
    max |q_T - q_0| <= 1e-3 rad; with zero efforts the robot sags by more than
    0.1 rad."""
    dof, dof0 = reference_loop("hold")
    free, _ = reference_loop("free")
    held, sag = float(np.abs(dof[:, 0] - dof0[:, 0]).max()), float(np.abs(free[:, 0] - dof0[:, 0]).max())
    print({"held": held, "free": sag, "held_speed": float(np.abs(dof[:, 1]).max())})
    assert held <= HOLD_BOUND
    assert sag > 0.1


def test_closed_loop_lets_moving_joints_coast():
    """(e) with the arm joints moving and both terms on, u' = 0: every joint
    velocity stays within 1e-3 rad/s of its start over the 60 steps while the
    arms travel about ARM_SPEED x 0.5 s; with the gravity term alone the
    Coriolis and centrifugal forces change the velocities by more than 0.1
    rad/s.  Measured: 3.4e-6 rad/s against 0.48 rad/s."""
    dof, dof0 = reference_loop("coast")
    grav, _ = reference_loop("coast_gravity")
    drift, ctrl = float(np.abs(dof[:, 1] - dof0[:, 1]).max()), float(np.abs(grav[:, 1] - dof0[:, 1]).max())
    moved = float(np.abs(dof[:, 0] - dof0[:, 0]).max())
    print({"coast_drift": drift, "gravity_only_drift": ctrl, "moved": moved})
    assert drift <= COAST_BOUND
    assert ctrl > 0.1
    assert moved > 0.4 * ARM_SPEED * CLOSED_LOOP_STEPS / 120.0
