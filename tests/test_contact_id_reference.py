"""The float64 reference of the contact-consistent inverse dynamics
(tests/contact_id_ref.py) is pinned before the kernel is held to it
(tests/test_gpu_contact_id.py): it satisfies the equation of motion with point
Jacobians taken independently from the oracle, a single contact carries the
unique wrench, the distribution is the minimiser of its cost, the shares do what
the header says, the result does not depend on the env's place on the grid, and
in closed loop with the fp64 oracle's physics step its torques hold a standing,
free-floating Thormang that collapses without them.  No GPU needed.

Tolerances.  (1) to (4) are float64 identities of the same arrays: 1e-12
relative (1e-9 for the load split, as the issue sets).  (6): see HOLD."""
import functools

import numpy as np
import pytest

from tests import physics_models as pm
from tests.contact_id_ref import contact_id_ref, contact_points, point_jacobians, skew, wrench_cost
from tests.id_ref import GRAVITY, Kinematics, id_ref
from tests.oracle_lib import physics_step, rigid_body_states
from tests.test_id_reference import FAR, _case
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.sim import contact_link_indices, load_model

N = 3
MODELS = ["thormang", "gogoro"]


def contacts_of(m, K, seed=3):
    """K contacts [(link, offset)]: the links that carry shapes first (thormang:
    the feet), then for thormang the arm end links, then any other link; offsets
    U(-0.1, 0.1) in the link frame."""
    names = [l.name for l in m.links]
    links = list(contact_link_indices(m))
    links += [names.index(x) for x in ("l_arm_end_link", "r_arm_end_link") if x in names]
    links += [l for l in range(len(names) - 1, 0, -1)]
    uniq = []
    for l in links:
        if l not in uniq:
            uniq.append(l)
    rs = np.random.default_rng(seed)
    return [(int(l), tuple(rs.uniform(-0.1, 0.1, 3))) for l in uniq[:K]]


def _ref(name, K, share=None, accel=True, moment_arm=0.1, **kw):
    m, root, dof, ms, arm, rs = _case(name)
    k = Kinematics(m, root, dof)
    a = rs.normal(0, 2.0, (N, 6 + m.num_dof)) if accel else None
    con = contacts_of(m, K)
    tau, lam, b, Jp = contact_id_ref(m, root, dof, con, share=share, moment_arm=moment_arm, accel=a, mass_scale=ms,
                                     armature=arm, kin=k, parts=True, **kw)
    return m, root, dof, ms, arm, k, a, con, tau, lam, b, Jp


def _oracle_point_jacobians(m, root, dof, k, con, p):
    """Jp [N, K, 6, 6 + D] as the oracle's velocity of the point per unit u, column by column
    (the way jacobian_ref gets its columns): v_com + w x (p - c) and w of the link."""
    n, D = root.shape[0], m.num_dof
    Jp = np.zeros((n, len(con), 6, 6 + D))
    for col in range(6 + D):
        r = np.array(k.root0, np.float32)
        d = np.array(dof, np.float32).reshape(n, D, 2)
        r[:, 7:13] = 0.0
        d[:, :, 1] = 0.0
        if col < 6:
            r[:, 7 + col] = 1.0
        else:
            d[:, col - 6, 1] = 1.0
        v = rigid_body_states(k.desc, r, np.ascontiguousarray(d.reshape(n * D, 2)))[..., 7:13].astype(np.float64)
        for e in range(n):
            for i, (l, _off) in enumerate(con):
                Jp[e, i, :3, col] = v[e, l, :3] + np.cross(v[e, l, 3:], p[e, i] - k.c[e, l])
                Jp[e, i, 3:, col] = v[e, l, 3:]
    return Jp


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("name", MODELS)
def test_equation_of_motion(name, K):
    """(1) b - tau - sum_k Jp_k^T lambda_k = 0 to 1e-12 of max |b|, Jp_k from the
    oracle's point velocities; the base rows of tau vanish on that scale; G_k has
    the header's form [[1, 0], [[r_k]x, 1]] about the root com."""
    m, root, dof, ms, arm, k, a, con, tau, lam, b, Jp = _ref(name, K)
    p = contact_points(k, con)
    Jo = _oracle_point_jacobians(m, root, dof, k, con, p)
    scale = np.abs(b).max()
    res = b - tau - np.einsum("ekic,eki->ec", Jo, lam)
    assert np.abs(res).max() <= 1e-12 * scale
    assert np.abs(tau[:, :6]).max() <= 1e-12 * scale and np.abs(tau[:, 6:]).max() > 1e-3 * scale
    assert (np.abs(lam).max(axis=2) > 1e-6 * scale).all()                   # every contact is loaded
    for e in range(N):
        for i in range(K):
            G = np.eye(6)
            G[3:, :3] = skew(p[e, i] - k.c[e, 0])
            assert np.abs(Jp[e, i, :, :6].T - G).max() <= 1e-6   # (the oracle's float32 columns)


@pytest.mark.parametrize("name", MODELS)
def test_one_contact_carries_the_unique_wrench(name):
    """(2) K = 1: lambda = G_1^-1 b[0:6] to 1e-12, whatever moment_arm and the share's value."""
    m, root, dof, ms, arm, k, a, con, tau, lam, b, Jp = _ref(name, 1)
    want = np.stack([np.linalg.solve(Jp[e, 0, :, :6].T, b[e, :6]) for e in range(N)])[:, None]
    scale = np.abs(want).max()
    assert np.abs(lam - want).max() <= 1e-12 * scale
    for arm_l, s in ((0.02, 1.0), (1.0, 0.3), (0.1, 5.0)):
        t2, l2 = contact_id_ref(m, root, dof, con, share=np.full((N, 1), s), moment_arm=arm_l, accel=a,
                                mass_scale=ms, armature=arm, kin=k)
        assert np.abs(l2 - want).max() <= 1e-12 * scale
        assert np.abs(t2 - tau).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("name", MODELS)
def test_the_distribution_is_the_minimiser(name, K):
    """(3) adding any of 20 random null-space directions of [G_1 ... G_K] keeps
    the base rows balanced to 1e-12 and raises the cost strictly."""
    rs = np.random.default_rng(17)
    share = rs.uniform(0.1, 1.0, (N, K))
    m, root, dof, ms, arm, k, a, con, tau, lam, b, Jp = _ref(name, K, share=share)
    cost = wrench_cost(lam, share, 0.1)
    for e in range(N):
        Gall = np.concatenate([Jp[e, i, :, :6].T for i in range(K)], axis=1)      # 6 x 6K
        _u, sv, vt = np.linalg.svd(Gall)
        null = vt[6:]                                                               # (6K - 6) x 6K
        assert null.shape[0] == 6 * K - 6 and sv.min() > 1e-3
        assert np.abs(Gall @ lam[e].reshape(-1) - b[e, :6]).max() <= 1e-12 * np.abs(b[e, :6]).max()
        for _ in range(20):
            dl = (null.T @ rs.normal(0, 1, null.shape[0])) * np.abs(lam[e]).max() * rs.uniform(1e-3, 1.0)
            l2 = lam[e] + dl.reshape(K, 6)
            assert np.abs(Gall @ l2.reshape(-1) - b[e, :6]).max() <= 1e-12 * np.abs(b[e, :6]).max() * 10
            assert wrench_cost(l2[None], share[e][None], 0.1)[0] > cost[e]


@pytest.mark.parametrize("name", MODELS)
def test_shares(name):
    """(4) a zero share unloads a contact exactly and the rest equals the call
    without it; all shares zero gives the plain inverse dynamics; scaling every
    share changes nothing; negative shares count as zero."""
    m, root, dof, ms, arm, k, a, con, tau, lam, b, Jp = _ref(name, 4)
    scale = np.abs(b).max()
    rs = np.random.default_rng(23)
    share = rs.uniform(0.1, 1.0, (N, 4))
    kw = dict(accel=a, mass_scale=ms, armature=arm, kin=k)
    share0 = share.copy()
    share0[:, 2] = 0.0
    t0, l0 = contact_id_ref(m, root, dof, con, share=share0, **kw)
    assert (l0[:, 2] == 0.0).all()
    t3, l3 = contact_id_ref(m, root, dof, [con[0], con[1], con[3]], share=share[:, [0, 1, 3]], **kw)
    assert np.abs(t0 - t3).max() <= 1e-12 * scale and np.abs(l0[:, [0, 1, 3]] - l3).max() <= 1e-12 * scale
    assert np.abs(t0 - tau).max() > 1e-3 * scale
    sneg = share0.copy()
    sneg[:, 2] = -0.5
    tn, ln = contact_id_ref(m, root, dof, con, share=sneg, **kw)
    assert np.array_equal(tn, t0) and np.array_equal(ln, l0)
    tz, lz = contact_id_ref(m, root, dof, con, share=np.zeros((N, 4)), **kw)
    plain = id_ref(m, root, dof, accel=a, mass_scale=ms, armature=arm, kin=k)
    assert np.array_equal(tz, plain) and (lz == 0.0).all()
    ts, ls = contact_id_ref(m, root, dof, con, share=share, **kw)
    t7, l7 = contact_id_ref(m, root, dof, con, share=7.0 * share, **kw)
    assert np.abs(t7 - ts).max() <= 1e-12 * scale and np.abs(l7 - ls).max() <= 1e-12 * scale


def test_load_split_on_a_symmetric_stance():
    """(4) shares (0.7, 0.3), thormang upright at rest with zero joint angles,
    gravity only, the two contact points mirrored in y about the plane of the
    CoM at the feet's height.  The forces sum to the weight.  The vertical
    forces split 0.7 : 0.3 of the weight to 1e-9 when moments are cheap
    (moment_arm 3000 m: the deviation is of order (half stance width /
    moment_arm)^2).  At a finite moment arm the minimiser trades part of the
    split against the feet's roll moments, exactly as the closed form of the
    header says for this stance:
        f_z,k = s_k (W / S + y_nx r_ky),  y_nx = -pm_y W / (sum_k s_k r_ky^2 + S l^2)
    with pm the share-weighted mean contact point and r_k = p_k - pm, y measured
    from the CoM's plane (the split is then 0.61 : 0.39 at a stance width of
    0.2 m).  This is asserted to 1e-6 of the weight at the default 0.1 m: the
    reference's lever arms come from the oracle's float32 Jacobian columns, good
    to 1.2e-7 m, while the closed form uses the CoM itself, and a lever error d
    moves f_z by s_k |r_ky| W d / (sum_k s_k r_ky^2 + S l^2) = 2.3 W d here;
    measured 3.7e-9 of the weight."""
    m = load_model("thormang")
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=1)
    k = Kinematics(m, root, dof, desc)
    mass = k.li[:, 0]
    com = (mass[:, None] * k.c[0]).sum(0) / mass.sum()
    W = mass.sum() * 9.81
    names = [l.name for l in m.links]
    feet = [names.index("l_leg_foot_link"), names.index("r_leg_foot_link")]
    rb = rigid_body_states(desc, k.root0, k.dof).astype(np.float64)
    half = 0.1
    z = min(k.o[0, feet[0], 2], k.o[0, feet[1], 2])
    con = []
    from tests.jacobian_ref import quat_R
    for l, sgn in zip(feet, (1.0, -1.0)):
        p = np.array([com[0], com[1] + sgn * half, z])
        con.append((l, tuple(quat_R(rb[0, l, 3:7]).T @ (p - k.o[0, l]))))
    s = np.array([[0.7, 0.3]])
    kw = dict(share=s, gravity=True, velocity=False, kin=k)
    tau, lam = contact_id_ref(m, root, dof, con, moment_arm=3000.0, **kw)
    assert abs(lam[0, :, 2].sum() - W) <= 1e-9 * W
    assert np.abs(lam[0, :, 2] - s[0] * W).max() <= 1e-9 * W
    tau, lam = contact_id_ref(m, root, dof, con, moment_arm=0.1, **kw)
    pm_y = 0.7 * half - 0.3 * half
    r_y = np.array([half, -half]) - pm_y
    ynx = -pm_y * W / ((s[0] * r_y ** 2).sum() + 0.1 ** 2)
    want = s[0] * (W + ynx * r_y)
    print({"weight": W, "f_z": lam[0, :, 2].tolist(), "closed_form": want.tolist()})
    assert abs(lam[0, :, 2].sum() - W) <= 1e-9 * W
    assert np.abs(lam[0, :, 2] - want).max() <= 1e-6 * W
    assert lam[0, 0, 2] > lam[0, 1, 2] > 0


def test_result_does_not_depend_on_the_env_position():
    """(5) an env copied to (300, -200, 1) gives an equal result."""
    m, root, dof, ms, arm, rs = _case("thormang", n=2)
    root[1], ms[1] = root[0], ms[0]
    dof.reshape(2, m.num_dof, 2)[1] = dof.reshape(2, m.num_dof, 2)[0]
    root[1, :3] = FAR
    tau, lam = contact_id_ref(m, root, dof, contacts_of(m, 4), mass_scale=ms)
    assert np.array_equal(tau[0], tau[1]) and np.array_equal(lam[0], lam[1])
    assert np.abs(tau[0]).max() > 1.0 and np.abs(lam[0]).max() > 1.0


# ---------------------------------------------------------------- closed loop with the fp64 oracle step
SETTLE_STEPS, HOLD_STEPS, CLOSED_LOOP_N = 240, 60, 2
ARM_OFFSET = 0.4   # rad, one arm joint of env 1, so that it is not symmetric
# the hold's largest joint drift over the 60 steps, measured with this file's fp64 loop: see
# test_closed_loop_holds_the_standing_robot; the bound is 2 x it
HOLD_MEASURED = 0.01213
HOLD = 2 * HOLD_MEASURED


def closed_loop_case(m):
    """The free-base Thormang of the ThormangWalk task at its default stance:
    default joint angles (env 1 with l_arm_sh_r offset by ARM_OFFSET), spawn
    height, PD gains and armature of the task cfg, dt 1/120 x 1 substep.
    Returns (desc, sp, root, dof, props, pt, vt)."""
    from thormang_isaacgym_amd.cfg import load_task_cfg
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_dof_props
    n, D = CLOSED_LOOP_N, m.num_dof
    cfg = load_task_cfg("ThormangWalk", num_envs=n)
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=n, dt=1.0 / 120.0, substeps=1, gravity=GRAVITY)
    wprops, _kp, default = walk_dof_props(m, cfg, n)
    props[:] = wprops
    root[:, 2] = float(cfg["env"].get("spawnHeight", 0.79))
    pt[:] = default
    pt[1, m.dof_names.index("l_arm_sh_r")] += ARM_OFFSET
    dof.reshape(n, D, 2)[:, :, 0] = pt
    return desc, sp, root, dof, props, pt, vt


def effort_mode(props):
    """Every DOF in drive mode 3 with zero gains and an effort limit of 1e4, in place."""
    props[abi.TG_PROP_DRIVE_MODE] = 3
    props[abi.TG_PROP_STIFFNESS] = 0.0
    props[abi.TG_PROP_DAMPING] = 0.0
    props[abi.TG_PROP_EFFORT] = 1e4
    return props


def feet_contacts(m):
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
    feet = walk_feet_indices(m)
    assert len(feet) == 2
    return [(int(l), (0.0, 0.0, 0.0)) for l in feet]


@functools.lru_cache(maxsize=None)
def reference_loop(mode):
    """The oracle loop: 240 settling steps under the PD drives, then 60 steps in
    effort mode with act = tau_ref[6:] ('hold') or zero efforts ('free').
    Returns (final dof, settled dof, the predicted wrenches of the first hold
    step [N, 2, 6], the weights [N]), read-only."""
    m = load_model("thormang")
    n, D = CLOSED_LOOP_N, m.num_dof
    desc, sp, root, dof, props, pt, vt = closed_loop_case(m)
    for _ in range(SETTLE_STEPS):
        physics_step(desc, sp, root, dof, props, pt, vt)
    dof0 = dof.copy()
    effort_mode(props)
    con = feet_contacts(m)
    first = None
    for _ in range(HOLD_STEPS):
        act = np.zeros((n, D), np.float32)
        if mode == "hold":
            tau, lam = contact_id_ref(m, root, dof, con, desc=desc)
            first = lam if first is None else first
            act[:] = tau[:, 6:]
        physics_step(desc, sp, root, dof, props, pt, vt, act=act)
    weight = np.full(n, np.asarray(abi.model_arrays(m)["link_inertia"], np.float64)[:, 0].sum() * 9.81)
    for x in (dof, dof0):
        x.setflags(write=False)
    return dof, dof0, first, weight


def test_closed_loop_holds_the_standing_robot():
    """(6) 60 steps of act = tau_ref[6:] with the two feet as contacts hold the
    settled stance to HOLD; with zero efforts the robot collapses by more than
    0.1 rad.  Measured with this loop: held 0.01213 rad (HOLD_MEASURED), free
    1.54 rad.  The drift is the leftover settling velocity amplified by the
    inverted-pendulum mode of a robot balancing without feedback, not an error
    of the torques; HOLD = 2 x the measured value.  Every predicted vertical
    foot force is positive and the two sum to the weight within 1 %."""
    dof, dof0, lam, weight = reference_loop("hold")
    free, _d0, _l, _w = reference_loop("free")
    held = float(np.abs(dof[:, 0] - dof0[:, 0]).max())
    sag = float(np.abs(free[:, 0] - dof0[:, 0]).max())
    print({"held": held, "free": sag, "f_z": lam[:, :, 2].tolist(), "weight": weight.tolist()})
    assert sag > 0.1
    assert held <= HOLD
    assert (lam[:, :, 2] > 0).all()
    assert (np.abs(lam[:, :, 2].sum(axis=1) - weight) <= 0.01 * weight).all()
