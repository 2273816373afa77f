"""float64 reference for the inertial measurement unit (tgsim.h tg_imu), a plain
numpy restatement of the header's definitions -- it shares no code with the
kernels.

Link poses and velocities come from the CPU oracle's rigid-body states with
the root at the origin (tests/oracle_lib.rigid_body_states, as
tests/height_scan_ref.frame_poses takes them): the link's quaternion, the
velocity of its centre of mass and its angular velocity.  The velocity of the
material point p_s = o_l + R_l offset_s is formed from the com velocity in
float64, v = v_com + w x R_l (offset_s - c_l).  Everything after the oracle is
float64.  The history is an explicit argument and the new one is returned.

Also here, because the CPU and the GPU test files share them: the sensors and
the two independent random states A and B of every case.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests.jacobian_ref import quat_R
from tests.oracle_lib import rigid_body_states
from thormang_isaacgym_amd import abi

WIDTH, HISTORY = 20, 8
ImuRef = namedtuple("ImuRef", ["out", "history", "R", "v", "w"])
# the slot groups the parity figures are taken over
GROUPS = {"quat": slice(0, 4), "gravity": slice(4, 7), "velocities": slice(7, 13), "accelerations": slice(13, 19)}


def sensor_kinematics(m, root, dof, sensors, desc=None):
    """(quat [N, S, 4], R [N, S, 3, 3], v [N, S, 3], w [N, S, 3]) float64: the links' unit quaternions and
    rotations, the world velocity of every sensor point and the links' world angular velocities.  ``sensors``:
    (link index, offset) pairs."""
    desc = desc or abi.ModelDesc(m)
    root = np.asarray(root, np.float32)
    r0 = root.copy()
    r0[:, :3] = 0.0                     # no absolute position enters
    rb = rigid_body_states(desc, r0, np.asarray(dof, np.float32)).astype(np.float64)
    com = np.asarray(abi.model_arrays(m)["link_inertia"], np.float64)[:, 1:4]
    n, S = root.shape[0], len(sensors)
    quat, R = np.zeros((n, S, 4)), np.zeros((n, S, 3, 3))
    v, w = np.zeros((n, S, 3)), np.zeros((n, S, 3))
    for e in range(n):
        for s, (l, off) in enumerate(sensors):
            quat[e, s] = rb[e, l, 3:7] / np.linalg.norm(rb[e, l, 3:7])
            R[e, s] = quat_R(quat[e, s])
            w[e, s] = rb[e, l, 10:13]
            v[e, s] = rb[e, l, 7:10] + np.cross(w[e, s], R[e, s] @ (np.asarray(off, np.float64) - com[l]))
    return quat, R, v, w


def imu_ref(m, root, dof, sensors, gravity=(0.0, 0.0, -9.81), history=None, dt=None, reset=None, bias=None,
            gyro_noise=0.0, accel_noise=0.0, normals=None, desc=None):
    """ImuRef(out [N, S, 20], history [N, S, 8] as the call leaves it, R, v, w), float64.  ``history``: [N, S, 8]
    or None; ``reset``: [N] or None; ``bias``: [N, S, 6] or None; ``normals``: the standard normals [N, S, 6] the
    sigmas multiply (needed when one is non-zero)."""
    quat, R, v, w = sensor_kinematics(m, root, dof, sensors, desc)
    n, S = v.shape[:2]
    g = np.asarray(gravity, np.float64)
    gn = np.linalg.norm(g)
    out, new = np.zeros((n, S, WIDTH)), np.zeros((n, S, HISTORY))
    for e in range(n):
        for s in range(S):
            Rt = R[e, s].T
            a, alpha, valid = np.zeros(3), np.zeros(3), 0.0
            if history is not None and float(history[e, s, 6]) == 1.0 and not (reset is not None and reset[e] != 0):
                a = (v[e, s] - np.asarray(history[e, s, 0:3], np.float64)) / float(dt)
                alpha = (w[e, s] - np.asarray(history[e, s, 3:6], np.float64)) / float(dt)
                valid = 1.0
            o = out[e, s]
            o[0:4] = quat[e, s]
            o[4:7] = Rt @ g / gn if gn > 0 else 0.0
            o[7:10] = Rt @ v[e, s]
            o[10:13] = Rt @ w[e, s]
            o[13:16] = Rt @ (a - g)
            o[16:19] = Rt @ alpha
            o[19] = valid
            if bias is not None:
                o[10:16] += np.asarray(bias[e, s], np.float64)
            if gyro_noise != 0.0 or accel_noise != 0.0:
                o[10:13] += float(gyro_noise) * np.asarray(normals[e, s, 0:3], np.float64)
                o[13:16] += float(accel_noise) * np.asarray(normals[e, s, 3:6], np.float64)
            new[e, s, 0:3], new[e, s, 3:6], new[e, s, 6], new[e, s, 7] = v[e, s], w[e, s], 1.0, 0.0
    return ImuRef(out, new, R, v, w)


def align_quat(got, ref):
    """``got`` [..., 4] with the sign of each quaternion turned to that of ``ref`` (q and -q are one rotation)."""
    sign = np.where((got * ref).sum(axis=-1, keepdims=True) < 0, -1.0, 1.0)
    return got * sign


# ---------------------------------------------------------------- the cases of the GPU tests
N = 5
FAR = (4000.0, -3000.0, 2.0)        # env 1's root: no absolute position may enter
DT = 0.01
CASES = ["thormang", "gogoro", "jit_walker", "kat_free", "thormang8"]


def case_model(case):
    from tests import physics_models as pm
    from thormang_isaacgym_amd.sim import load_model
    name = "thormang" if case == "thormang8" else case
    return {"jit_walker": pm.jit_walker, "kat_free": pm.free_body}.get(name, lambda: load_model(name))()


def case_sensors(case, m):
    """(link index, offset) pairs of a case."""
    if case in ("thormang", "thormang8"):
        from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
        lf, rf = walk_feet_indices(m)
        imu = m.link_index("imu_link")
        three = [(imu, (0.0, 0.0, 0.0)), (lf, (0.05, 0.01, -0.03)), (rf, (-0.02, 0.03, -0.03))]
        if case == "thormang":
            return three
        last = m.num_bodies - 1          # eight sensors: the root, a repeated link and the last link among them
        return three + [(0, (0.0, 0.0, 0.0)), (imu, (0.1, -0.2, 0.3)), (last, (0.0, 0.0, 0.0)),
                        (last, (0.02, 0.0, -0.01)), (m.num_bodies // 2, (0.0, 0.05, 0.0))]
    if case == "gogoro":
        return [(0, (0.0, 0.0, 0.0))]
    if case == "jit_walker":
        return [(0, (0.0, 0.0, 0.0)), (m.num_bodies - 1, (0.1, 0.0, -0.05))]
    return [(0, (0.2, -0.1, 0.05)), (0, (0.0, 0.0, 0.0))]        # kat_free: one link in two sensors


def scenario(case, n=N, seed=71):
    """(model, sensors, (root A, dof A), (root B, dof B)): two independent random_state draws; env 1 stands at FAR
    in both.  No GPU needed."""
    from tests.test_rigid_body_states import random_state
    m = case_model(case)
    rs = np.random.default_rng(seed)
    A, B = random_state(m, n, rs), random_state(m, n, rs)
    if n > 1:
        A[0][1, :3] = FAR
        B[0][1, :3] = FAR
    return m, case_sensors(case, m), A, B
