"""Small analytic articulations for the physics known-answer tests (CPU oracle
and GPU kernel alike).  Built from URDF text with the product's own URDF
loader, so the same model path is exercised."""
from __future__ import annotations

import numpy as np

from thormang_isaacgym_amd.abi import ModelDesc, default_dof_props, sim_params_from_cfg


from thormang_isaacgym_amd.model.kat_models import box_body, chain, free_body, pendulum, sphere_body, urdf_model  # noqa: F401


def sim(m, n=1, dt=0.01, substeps=1, gravity=(0, 0, -9.81), solver_type=0, **ao):
    sp = sim_params_from_cfg({"dt": dt, "substeps": substeps, "gravity": list(gravity),
                              "physx": {"rest_offset": 0.0, "max_depenetration_velocity": 1.0,
                                        "solver_type": solver_type}},
                             dict(dict(angular_damping=0.0, linear_damping=0.0, contact_iterations=16), **ao), n)
    desc = ModelDesc(m)
    D = m.num_dof
    props = default_dof_props(m, n)
    root = np.zeros((n, 13), np.float32)
    root[:, 6] = 1.0
    dof = np.zeros((n * D, 2), np.float32)
    pt = np.zeros((n, D), np.float32)
    vt = np.zeros((n, D), np.float32)
    return desc, sp, root, dof, props, pt, vt


def _rpy_free_R(o):
    return np.asarray(o, np.float64)


def system_com(m, root, q):
    """World COM of an articulation from the root state and dof positions (plain numpy FK)."""
    from thormang_isaacgym_amd.model.urdf import JOINT_PRISMATIC, JOINT_REVOLUTE
    x, y, z, w = [float(v) for v in root[3:7]]
    R0 = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Rs, ps = [], []
    tot, acc = 0.0, np.zeros(3)
    for i, l in enumerate(m.links):
        if l.parent < 0:
            R, p = R0, np.asarray(root[0:3], np.float64)
        else:
            j = m.joints[l.joint]
            Ro, to = np.asarray(j.origin_rot), np.asarray(j.origin_pos, np.float64)
            a = np.asarray(j.axis)
            if j.jtype == JOINT_REVOLUTE:
                th = float(q[j.dof])
                K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                Ro = Ro @ (np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K)
            elif j.jtype == JOINT_PRISMATIC:
                to = to + Ro @ a * float(q[j.dof])
            R, p = Rs[l.parent] @ Ro, ps[l.parent] + Rs[l.parent] @ to
        Rs.append(R)
        ps.append(p)
        acc += l.mass * (p + R @ np.asarray(l.com))
        tot += l.mass
    return acc / tot


def drop_box(solver_type, iters=4, viters=1, rest_offset=0.0, z0=0.25, steps=90, dt=1.0 / 60.0, substeps=2,
             step_fn=None, contact_offset=None, vz0=0.0):
    """A 0.1 m box (kat_models.box_body, half height 0.05) released at rest
    ``z0`` above the ground under gravity, with the walk cfg's solver
    (cfg/task/ThormangWalk.yaml: dt 1/60 x 2 substeps, TGS 4 position + 1
    velocity iterations).  Returns the per-step root height and vertical
    velocity.  ``step_fn(desc, sp, root, dof, props, pt, vt)`` steps one env
    (default: the CPU oracle).  ``contact_offset`` sets sim.physx's key (None:
    the default), ``vz0`` the initial vertical velocity."""
    from tests.oracle_lib import physics_step
    m = box_body(mu=0.8)
    sp = sim_params_from_cfg({"dt": dt, "substeps": substeps, "gravity": [0, 0, -9.81],
                              "physx": {"num_position_iterations": iters, "num_velocity_iterations": viters,
                                        "rest_offset": rest_offset, "max_depenetration_velocity": 1.0,
                                        "solver_type": solver_type,
                                        **({} if contact_offset is None else {"contact_offset": contact_offset})}},
                             dict(angular_damping=0.0, linear_damping=0.0, ground_friction=0.8), 1, warn=False)
    desc = ModelDesc(m)
    props = default_dof_props(m, 1)
    root = np.zeros((1, 13), np.float32)
    root[0, 2] = z0
    root[0, 6] = 1.0
    root[0, 9] = vz0
    dof = np.zeros((0, 2), np.float32)
    z = np.zeros((1, 0), np.float32)
    step = step_fn or physics_step
    zs, vs = [], []
    for _ in range(steps):
        step(desc, sp, root, dof, props, z, z)
        zs.append(float(root[0, 2]))
        vs.append(float(root[0, 9]))
    return np.array(zs), np.array(vs)


def landing_checks(zs, vs, rest_offset=0.0, half=0.05):
    """What the physics itself requires of a restitution-0 landing, whatever
    the solver's internals: once the box has reached the ground
    it never moves up again by more than 0.5 mm nor leaves with an upward
    velocity over 2 cm/s (no rebound), it never sinks more than 2 mm below
    its rest height, and it comes to rest at half height + rest offset
    within 0.5 mm, at rest within 1 mm/s.  Returns a dict of the measured
    quantities and ``ok``."""
    rest = half + rest_offset
    hit = int(np.argmax(zs < rest + 0.002))
    after = zs[hit:]
    out = {"hit_step": hit, "rise_after_hit": float(after.max() - after[0]) if len(after) else 0.0,
           "max_up_velocity": float(vs[hit:].max()), "min_height": float(zs.min()) - rest,
           "final_height": float(zs[-1]) - rest, "final_vz": float(vs[-1])}
    out["ok"] = bool(hit > 0 and zs[hit - 1] > rest + 0.002 and out["rise_after_hit"] < 5e-4 and
                     out["max_up_velocity"] < 0.02 and out["min_height"] > -0.002 and
                     abs(out["final_height"]) < 5e-4 and abs(out["final_vz"]) < 1e-3)
    return out


# ---------------------------------------------------------------- drive / limit / friction known answers
# One env each; ``step_fn(desc, sp, root, dof, props, pt, vt)`` steps it in place
# (default: the CPU oracle), ``make_step()`` returns a fresh one per run.  The
# helpers return what was measured; the tests assert (CPU: test_physics_oracle,
# GPU: test_gpu_drive_limits, the same bounds).
def run_steps(state, steps, record, step_fn=None):
    from tests.oracle_lib import physics_step
    desc, sp, root, dof, props, pt, vt = state
    step = step_fn or physics_step
    out = []
    for _ in range(steps):
        step(desc, sp, root, dof, props, pt, vt)
        out.append(record(root, dof))
    return np.array(out)


def velocity_drive_runs(make_step=None):
    """A velocity drive (kd 1000) on the pendulum about z, dt 0.01 x 2
    substeps: the joint velocity over 20 steps towards 7 rad/s with effort 1e6,
    and over 10 steps (0.1 s) towards 100 rad/s with effort 0.5 -- constant
    acceleration effort / I, I = 0.01 (the COM lies on the axis).  Returns the
    two velocity traces."""
    from thormang_isaacgym_amd.abi import TG_PROP_DAMPING, TG_PROP_DRIVE_MODE, TG_PROP_EFFORT
    mk = make_step or (lambda: None)
    out = []
    for effort, target, steps in ((1e6, 7.0, 20), (0.5, 100.0, 10)):
        st = sim(pendulum(axis="0 0 1"), dt=0.01, substeps=2, fix_base_link=True)
        desc, sp, root, dof, props, pt, vt = st
        props[TG_PROP_DRIVE_MODE, 0, 0] = 2
        props[TG_PROP_DAMPING, 0, 0] = 1000.0
        props[TG_PROP_EFFORT, 0, 0] = effort
        vt[0, 0] = target
        out.append(run_steps(st, steps, lambda r, d: d[0, 1], mk()))
    return out


def position_drive_run(step_fn=None):
    """A position drive (kp 3000, kd 300) on the pendulum about z towards
    0.4 rad: the joint angle over 100 steps."""
    from thormang_isaacgym_amd.abi import TG_PROP_DAMPING, TG_PROP_DRIVE_MODE, TG_PROP_EFFORT, TG_PROP_STIFFNESS
    st = sim(pendulum(axis="0 0 1"), dt=0.01, substeps=2, fix_base_link=True)
    desc, sp, root, dof, props, pt, vt = st
    props[TG_PROP_DRIVE_MODE, 0, 0] = 1
    props[TG_PROP_STIFFNESS, 0, 0] = 3000.0
    props[TG_PROP_DAMPING, 0, 0] = 300.0
    props[TG_PROP_EFFORT, 0, 0] = 1e6
    pt[0, 0] = 0.4
    return run_steps(st, 100, lambda r, d: d[0, 0], step_fn)


def joint_limit_run(step_fn=None, through_props=False):
    """The pendulum about y with a +-0.3 rad window, its fixed base tilted so
    that gravity swings the arm towards +-pi/2: the joint angle over 300 steps.
    The window comes from the URDF, or (``through_props``) is set in dof_props
    on the compiled-in continuous-joint model."""
    from thormang_isaacgym_amd.abi import TG_PROP_LOWER, TG_PROP_UPPER
    st = sim(pendulum() if through_props else pendulum(limits=(-0.3, 0.3)), dt=0.01, substeps=2, fix_base_link=True)
    if through_props:
        st[4][TG_PROP_LOWER, 0, 0], st[4][TG_PROP_UPPER, 0, 0] = -0.3, 0.3
    st[3][0, 0] = 0.0
    st[2][0, 3:7] = [0, np.sin(0.7), 0, np.cos(0.7)]   # tilt the fixed base so gravity has a lever arm
    return run_steps(st, 300, lambda r, d: d[0, 0], step_fn)


def coulomb_slide_run(step_fn=None, mu=0.5, model=None):
    """A box sliding at 2 m/s on friction ``mu``: (x, vx) over 200 steps and
    the expected stopping distance v^2 / (2 mu g).  ``model``: the box to use
    (default: one built with shape friction ``mu``; the caller of another sets
    the shape friction at run time)."""
    st = sim(model or box_body(mu=mu), dt=0.005, substeps=1, ground_friction=mu)
    st[2][0, 2] = 0.05
    st[2][0, 7] = 2.0
    return run_steps(st, 200, lambda r, d: r[0, [0, 7]].copy(), step_fn), 2.0 ** 2 / (2 * mu * 9.81)


def chain_internal_drive_run(step_fn=None):
    """Zero gravity, no contact, a velocity drive (kd 5, target 4 rad/s) on the
    chain's revolute joint: per step the system COM (3) and the joint
    velocities (2), 500 steps."""
    from thormang_isaacgym_amd.abi import TG_PROP_DAMPING, TG_PROP_DRIVE_MODE, TG_PROP_EFFORT
    m = chain()
    st = sim(m, dt=0.002, substeps=1, gravity=(0, 0, 0))
    desc, sp, root, dof, props, pt, vt = st
    props[TG_PROP_DRIVE_MODE, 0, 0] = 2
    props[TG_PROP_DAMPING, 0, 0] = 5.0
    props[TG_PROP_EFFORT, 0, 0] = 1e9
    vt[0, 0] = 4.0
    return run_steps(st, 500, lambda r, d: np.concatenate([system_com(m, r[0], d[:, 0]), d[:, 1]]), step_fn)


def limit_ramp():
    """TG_LIMIT_RAMP as include/tgsim.h defines it."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "tgsim.h")) as f:
        return float(re.search(r"#define\s+TG_LIMIT_RAMP\s+([0-9.eE+-]+)f?", f.read()).group(1))


def dof_tree(desc):
    """Per DOF of a model descriptor: its group and whether that group is a
    leaf of the group tree (no other group has it as parent)."""
    a = desc.arrays
    parent = np.asarray(a["group_parent"])
    dof_of_group = np.asarray(a["link_dof"])[np.asarray(a["group_root"])]
    D = len(a["dof_locked"])
    group, leaf = np.full(D, -1), np.zeros(D, bool)
    for g in range(1, len(parent)):
        group[dof_of_group[g]] = g
        leaf[dof_of_group[g]] = g not in set(parent.tolist())
    return group, leaf


def jit_walker():
    """A URDF that is not compiled into libtgsim.so (run-time load_asset /
    tg_model_jit test): a box torso with two legs, hips driven, one knee
    locked, sphere feet and a box body shape."""
    from thormang_isaacgym_amd.model.kat_models import _inertial, urdf_model
    from thormang_isaacgym_amd.model.urdf import Shape
    eye = np.eye(3).tolist()
    legs = ""
    for side, y in (("l", 0.12), ("r", -0.12)):
        legs += (f'<link name="{side}_thigh">{_inertial(0.8, (0, 0, -0.15), (0.006, 0.006, 0.001))}</link>'
                 f'<link name="{side}_shin">{_inertial(0.5, (0, 0, -0.12), (0.003, 0.003, 0.0005))}</link>'
                 f'<joint name="{side}_hip" type="revolute"><parent link="torso"/><child link="{side}_thigh"/>'
                 f'<origin xyz="0 {y} -0.1" rpy="0.05 0 0"/><axis xyz="0 1 0"/>'
                 '<limit lower="-1.2" upper="1.2" effort="80" velocity="10"/></joint>'
                 f'<joint name="{side}_knee" type="revolute"><parent link="{side}_thigh"/><child link="{side}_shin"/>'
                 '<origin xyz="0 0 -0.3"/><axis xyz="0 1 0"/>'
                 '<limit lower="-0.5" upper="1.5" effort="80" velocity="10"/></joint>')
    shapes = [Shape("box", "torso", [0, 0, 0], eye, [0.12, 0.18, 0.1], 0.9),
              Shape("sphere", "l_shin", [0, 0, -0.26], eye, [0.04], 1.0),
              Shape("sphere", "r_shin", [0, 0, -0.26], eye, [0.04], 1.0)]
    return urdf_model("jit_walker", f'<link name="torso">{_inertial(4.0, (0, 0, 0.02), (0.05, 0.04, 0.03))}</link>'
                      + legs, shapes, locked=["r_knee"])


def contact_offset_checks(make_step=None, solver_type=1, contact_offset=0.02):
    """Known answers of the contact_offset gate, for the oracle or
    the GPU (``make_step()`` returns a fresh drop_box ``step_fn`` per run),
    with the walk cfg's step (dt 1/60 x 2 substeps, h = 1/120) and
    contact_margin 0.05.  The rule is PhysX's: a contact exists while the
    separation is below the pair's contact distance, the shape's plus the
    ground plane's offset (2 x 0.02 = 4 cm here).

    * ``rest_gap``: a box at rest 4.5 cm up (beyond the pair distance, within
      the margin) takes no normal impulse -- one step is the exact
      semi-implicit free fall, z0 - 3 g h^2, vz = -2 g h;
    * ``fast``: a box 3.5 cm up (inside the pair distance) approaching at
      6 m/s (0.05 m per substep) has its speculative row and lands on the
      ground in the first substep (free flight would end 1.6 cm below it);
    * ``beyond``: the same approach from 4.5 cm up has no row in the first
      substep (PhysX without CCD: it passes the surface by ~6 mm), then the
      row and the push-out bring it back to rest.
    Returns a dict of the measured quantities."""
    g, h, half = 9.81, 1.0 / 120.0, 0.05
    mk = make_step or (lambda: None)
    z0 = half + 0.045
    zs, vs = drop_box(solver_type, z0=z0, steps=1, step_fn=mk(), contact_offset=contact_offset)
    out = {"rest_gap_dz": float(zs[0] - (z0 - 3 * g * h * h)), "rest_gap_dvz": float(vs[0] + 2 * g * h)}
    z0 = half + 0.035
    zs, vs = drop_box(solver_type, z0=z0, steps=20, step_fn=mk(), contact_offset=contact_offset, vz0=-6.0)
    out.update(fast_min_z=float(zs.min()) - half, fast_z1=float(zs[0]) - half, fast_vz1=float(vs[0]),
               fast_final=float(zs[-1]) - half, free_flight_z1=float(z0 - 2 * 6.0 * h - 3 * g * h * h) - half)
    z0 = half + 0.045
    zs, vs = drop_box(solver_type, z0=z0, steps=40, substeps=2, step_fn=mk(), contact_offset=contact_offset,
                      vz0=-6.0)
    out.update(beyond_min_z=float(zs.min()) - half, beyond_final=float(zs[-1]) - half, beyond_vz_final=float(vs[-1]))
    return out
