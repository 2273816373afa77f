"""The float64 reference of the operational-space control (tests/osc_ref.py)
means what include/tgsim.h says: at damping 0 it is the reference task's
literal formula (tasks/franka_cube_stack.py:602-628), its torques produce
exactly the commanded task acceleration and its null-space part none, it does
not depend on where the env sits, and in closed loop with the fp64 oracle's
physics step it brings a hand and a foot to their goals.  No GPU needed; the
kernel is held to this reference in tests/test_gpu_osc.py."""
import numpy as np
import pytest

from tests import physics_models as pm
from tests.ik_ref import link_pose_goal, path_dofs, pose_error
from tests.oracle_lib import physics_step
from tests.osc_ref import chain_blocks, null_acceleration, osc_ref, osc_torques
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.sim import load_model

FAR = (300.0, -200.0, 1.0)
KP, KP_NULL = 150.0, 10.0
KD, KD_NULL = 2.0 * np.sqrt(KP), 2.0 * np.sqrt(KP_NULL)
# (link, chain = the last nd DOFs on its path, seed)
CLOSED_LOOP_CASES = [("l_arm_end_link", 7, 7), ("r_leg_foot_link", 6, 4)]
CLOSED_LOOP_STEPS, CLOSED_LOOP_DAMPING = 120, 1e-2


def _chain(m, link_name, nd):
    link = m.link_index(link_name)
    return (link, path_dofs(m, link)[-nd:], (0.0, 0.0, 0.0))


def _armature(m, n, rs):
    return rs.uniform(0.005, 0.02, (n, m.num_dof)).astype(np.float32)


def error_norms(err):
    return np.linalg.norm(err[:, :3], axis=1), np.linalg.norm(err[:, 3:], axis=1)


def test_reference_equals_the_reference_tasks_literal_formula():
    """_compute_osc_torques line by line in numpy, on the left arm's 7 DOFs; eef_vel = J qd (base held)."""
    m = load_model("thormang")
    n, D = 3, m.num_dof
    rs = np.random.default_rng(2)
    root, dof = random_state(m, n, rs)
    chain = _chain(m, "l_arm_end_link", 7)
    arm = _armature(m, n, rs)
    gp = (root[:, None, :3] + rs.uniform(-0.3, 0.3, (n, 1, 3))).astype(np.float32)
    gq = rs.normal(0, 1, (n, 1, 4)).astype(np.float32)
    rest = rs.uniform(-4.0, 4.0, (n, D)).astype(np.float32)         # some differences beyond +-pi: the wrap acts
    tau, err = osc_ref(m, root, dof, [chain], gp, gq, q_rest=rest, kp=KP, kp_null=KP_NULL, damping=0.0, armature=arm)
    assert (tau[:, 0, 7:] == 0.0).all()
    (blocks,), _frames = chain_blocks(m, root, dof, [chain], armature=arm)
    s = dof.reshape(n, D, 2).astype(np.float64)
    wrapped = 0
    for e in range(n):
        j_eef, mm = blocks[0][e], blocks[1][e]
        q, qd = s[e, chain[1], 0], s[e, chain[1], 1]
        dpose, eef_vel = err[e, 0], j_eef @ qd
        mm_inv = np.linalg.inv(mm)
        m_eef_inv = j_eef @ mm_inv @ j_eef.T
        m_eef = np.linalg.inv(m_eef_inv)
        u = j_eef.T @ m_eef @ (KP * dpose - KD * eef_vel)
        j_eef_inv = m_eef @ j_eef @ mm_inv
        d = rest[e, chain[1]].astype(np.float64) - q
        wrapped += int((np.abs(d) > np.pi).sum())
        u_null = KD_NULL * -qd + KP_NULL * ((d + np.pi) % (2 * np.pi) - np.pi)
        u_null = mm @ u_null
        u += (np.eye(7) - j_eef.T @ j_eef_inv) @ u_null
        np.testing.assert_allclose(tau[e, 0, :7], u, rtol=0, atol=1e-9 * np.abs(u).max())
    assert wrapped > 0


@pytest.mark.parametrize("link_name,nd", [("l_arm_end_link", 7), ("r_leg_foot_link", 6), ("r_arm_end_link", 8)])
def test_torques_decouple_task_and_null_space(link_name, nd):
    """At damping 0 with nd >= 6: the task acceleration J H_c^-1 tau is kp err
    - kd v, and the null-space part adds none."""
    m = load_model("thormang")
    n, D = 3, m.num_dof
    rs = np.random.default_rng(5)
    root, dof = random_state(m, n, rs)
    chain = _chain(m, link_name, nd)
    arm = _armature(m, n, rs)
    scale = rs.uniform(0.8, 1.2, (n, m.num_bodies)).astype(np.float32)
    gp = (root[:, :3] + rs.uniform(-0.3, 0.3, (n, 3))).astype(np.float32)
    gq = rs.normal(0, 1, (n, 4)).astype(np.float32)
    rest = rs.uniform(-1.0, 1.0, (n, D)).astype(np.float32)
    (blocks,), frames = chain_blocks(m, root, dof, [chain], mass_scale=scale, armature=arm)
    err = pose_error(m, root, dof, chain, gp, gq, frames=frames)
    a = null_acceleration(m, dof, chain[1], rest, KP_NULL, KD_NULL)
    qd = dof.reshape(n, D, 2)[:, chain[1], 1].astype(np.float64)
    for e in range(n):
        J, H = blocks[0][e], blocks[1][e]
        tau, task, null = osc_torques(J, H, err[e], qd[e], KP, KD, 0.0, a[e])
        want = KP * err[e] - KD * (J @ qd[e])
        acc_task, acc_null = J @ np.linalg.solve(H, task), J @ np.linalg.solve(H, null)
        s = np.abs(want).max()
        print({"link": link_name, "env": e, "task_residual": float(np.abs(acc_task - want).max() / s),
               "null_task_acc": float(np.abs(acc_null).max() / s), "null_torque": float(np.abs(null).max())})
        assert np.abs(acc_task - want).max() <= 1e-9 * s
        assert np.abs(acc_null).max() <= 1e-9 * max(s, np.abs(J @ a[e]).max())
        if nd > 6:
            assert np.abs(null).max() > 1e-3                            # (there is a null-space torque)
        else:
            assert np.abs(null).max() <= 1e-9 * np.abs(H @ a[e]).max()   # (a square J leaves no null space)
        np.testing.assert_allclose(tau, task + null, rtol=0, atol=0)


def test_result_does_not_depend_on_the_env_position():
    """Two envs in the same state, one far out on the grid, goals at the same
    place relative to the root (offsets on a 2^-10 grid, so the float32 world
    goals are exact in both): the same torques."""
    m = load_model("thormang")
    D = m.num_dof
    rs = np.random.default_rng(1)
    root, dof = random_state(m, 2, rs)
    root[:, :3] = 0.0
    root[1] = root[0]
    dof.reshape(2, D, 2)[1] = dof.reshape(2, D, 2)[0]
    root[1, :3] = FAR
    chains = [_chain(m, "l_arm_end_link", 7), _chain(m, "r_leg_foot_link", 6)]
    rel = np.round(rs.uniform(-0.5, 0.5, (1, 2, 3)) * 1024) / 1024
    gp = (root[:, None, :3].astype(np.float64) + rel).astype(np.float32)
    assert np.array_equal(gp[1].astype(np.float64) - np.asarray(FAR), gp[0].astype(np.float64))
    gq = np.repeat(rs.normal(0, 1, (1, 2, 4)), 2, axis=0).astype(np.float32)
    rest = np.repeat(rs.uniform(-1, 1, (1, D)), 2, axis=0).astype(np.float32)
    arm = np.repeat(_armature(m, 1, rs), 2, axis=0)
    tau, err = osc_ref(m, root, dof, chains, gp, gq, q_rest=rest, armature=arm)
    np.testing.assert_allclose(tau[1], tau[0], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(err[1], err[0], rtol=0, atol=1e-12)
    assert np.abs(tau[0]).max() > 1.0


def closed_loop_case(m, link_name, nd, seed, n=3):
    """The closed-loop setup: the fixed-base Thormang at z = 2 without gravity,
    dt 1/120 x 1 substep, armature 0.01; the chain DOFs in EFFORT mode with
    zero gains, every other DOF position-driven (kp 1000, kd 50) at its start;
    positions at lower + U(0.3, 0.7) (upper - lower), at rest; the goal the
    link's pose at q + U(-0.25, 0.25) on the chain.  Returns (state, chain, gp
    [N, 3], gq [N, 4]) with state = (desc, sp, root, dof, props, pt, vt)."""
    rs = np.random.default_rng(seed)
    D = m.num_dof
    st = pm.sim(m, n=n, dt=1.0 / 120.0, substeps=1, gravity=(0, 0, 0), fix_base_link=True)
    desc, sp, root, dof, props, pt, vt = st
    root[:, 2] = 2.0
    chain = _chain(m, link_name, nd)
    lo, hi = props[abi.TG_PROP_LOWER].astype(np.float64), props[abi.TG_PROP_UPPER].astype(np.float64)
    assert (np.abs(lo) < 1e30).all() and (np.abs(hi) < 1e30).all()
    q0 = (lo + rs.uniform(0.3, 0.7, (n, D)) * (hi - lo)).astype(np.float32)
    dof.reshape(n, D, 2)[:, :, 0] = q0
    pt[:] = q0
    props[abi.TG_PROP_ARMATURE] = 0.01
    props[abi.TG_PROP_DRIVE_MODE] = 1
    props[abi.TG_PROP_STIFFNESS] = 1000.0
    props[abi.TG_PROP_DAMPING] = 50.0
    for f, v in ((abi.TG_PROP_DRIVE_MODE, 3), (abi.TG_PROP_STIFFNESS, 0.0), (abi.TG_PROP_DAMPING, 0.0)):
        props[f][:, chain[1]] = v
    moved = dof.reshape(n, D, 2).copy()
    moved[:, chain[1], 0] += rs.uniform(-0.25, 0.25, (n, nd)).astype(np.float32)
    gp, gq = link_pose_goal(m, root, np.ascontiguousarray(moved.reshape(n * D, 2)), chain)
    return st, chain, gp, gq


@pytest.mark.parametrize("link_name,nd,seed", CLOSED_LOOP_CASES)
def test_closed_loop_with_the_oracle_reaches_the_goal(link_name, nd, seed):
    """120 steps of osc_ref -> clamp to the effort limits -> the fp64 oracle's
    physics step: both error norms end at <= 10 % of their initial value in
    every env.  Measured: arm 0.023 % / 3.5 %, foot 0.024 % / 3.5 % (position /
    orientation: the quaternion's vector part is half the angle, so the
    orientation loop has stiffness 75 under the damping 2 sqrt(150) and its
    slow pole -12.25 + sqrt(75) = -3.6 / s leaves exp(-3.6) = 2.8 % after 1 s),
    the largest torque 6.3 % of the 1000 N m effort limit."""
    m = load_model("thormang")
    n, D = 3, m.num_dof
    (desc, sp, root, dof, props, pt, vt), chain, gp, gq = closed_loop_case(m, link_name, nd, seed, n)
    rest = dof.reshape(n, D, 2)[:, :, 0].copy()
    p0, o0 = error_norms(pose_error(m, root, dof, chain, gp, gq, desc))
    effort = props[abi.TG_PROP_EFFORT].astype(np.float64)
    worst = 0.0
    for _ in range(CLOSED_LOOP_STEPS):
        tau, _err = osc_ref(m, root, dof, [chain], gp[:, None], gq[:, None], q_rest=rest, kp=KP, kp_null=KP_NULL,
                            damping=CLOSED_LOOP_DAMPING, armature=props[abi.TG_PROP_ARMATURE], desc=desc)
        act = np.zeros((n, D), np.float32)
        act[:, chain[1]] = np.clip(tau[:, 0, :nd], -effort[:, chain[1]], effort[:, chain[1]])
        worst = max(worst, float((np.abs(tau[:, 0, :nd]) / effort[:, chain[1]]).max()))
        physics_step(desc, sp, root, dof, props, pt, vt, act=act)
    p1, o1 = error_norms(pose_error(m, root, dof, chain, gp, gq, desc))
    print({"link": link_name, "pos": (float(p0.max()), float(p1.max())), "orn": (float(o0.max()), float(o1.max())),
           "worst_ratio": (float((p1 / p0).max()), float((o1 / o0).max())), "worst_tau_over_effort": worst})
    assert (p1 <= 0.10 * p0).all() and (o1 <= 0.10 * o0).all(), (p0, p1, o0, o1)
