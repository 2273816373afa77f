"""float64 reference for the damped-least-squares IK (tgsim.h tg_ik_dls), built
only from the CPU oracle through tests/jacobian_ref.py and
tests/oracle_lib.rigid_body_states -- it shares no code with the kernel.

The controlled point of a chain is x = o_l + R_l offset, o_l the link ORIGIN
(rigid_body_states [0:3]).  jacobian_ref's linear rows are those of the link's
centre of mass c_l, so the point's rows are Jv_x = Jv_com - [x - c_l]x Jw.  The
pose error and the step are the header's:
    err[0:3] = (goal_pos - root_pos) - (x - root_pos)
    err[3:6] = vec(q_goal (x) conj(q_l)) s,  s = +1 if w >= 0 else -1
    dq       = J^T (J J^T + lambda^2 I)^-1 err     (rows 0..2 only without goal_quat)

The float32 root, dof and goal arrays are taken as given and everything after
the oracle is float64.  The oracle is evaluated with the root link at the
origin (the link poses relative to the root do not depend on where the env
sits), so its float32 output keeps its digits for an env far out on the grid;
the root position enters only through goal_pos - root_pos, in float64."""
from __future__ import annotations

import numpy as np

from tests.jacobian_ref import jacobian_ref, quat_R
from tests.oracle_lib import rigid_body_states
from thormang_isaacgym_amd import abi

MAX_DOFS = 8


def chain_spec(c):
    """(link, [dofs], offset) from such a tuple or from an abi.tg_ik_chain"""
    if isinstance(c, abi.tg_ik_chain):
        return int(c.link), [int(c.dofs[i]) for i in range(c.num_dofs)], [float(v) for v in c.offset]
    link, dofs, offset = c
    return int(link), [int(d) for d in dofs], [float(v) for v in offset]


def _at_origin(root):
    r = np.array(root, np.float32)
    r[:, :3] = 0.0
    return r


def link_frames(m, root, dof, desc=None):
    """(o [N, L, 3], q [N, L, 4], c [N, L, 3]) float64: link origins and centres of mass
    relative to the root link's origin (world axes), and the link quaternions xyzw."""
    desc = desc or abi.ModelDesc(m)
    rb = rigid_body_states(desc, _at_origin(root), np.asarray(dof, np.float32)).astype(np.float64)
    com = np.asarray(abi.model_arrays(m)["link_inertia"], np.float64)[:, 1:4]
    o, q = rb[..., 0:3], rb[..., 3:7]
    c = np.zeros_like(o)
    for e in range(o.shape[0]):
        for l in range(o.shape[1]):
            c[e, l] = o[e, l] + quat_R(q[e, l]) @ com[l]
    return o, q, c


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def point_jacobian(m, root, dof, chain, desc=None, J=None, frames=None):
    """[N, 6, nd] float64: the rows (Jv_x, Jw) of the chain's controlled point over the chain's DOF columns."""
    desc = desc or abi.ModelDesc(m)
    link, dofs, offset = chain_spec(chain)
    J = jacobian_ref(m, _at_origin(root), dof, desc) if J is None else J
    o, q, c = frames or link_frames(m, root, dof, desc)
    n = J.shape[0]
    out = np.zeros((n, 6, len(dofs)))
    cols = [6 + d for d in dofs]
    for e in range(n):
        x = o[e, link] + quat_R(q[e, link]) @ np.asarray(offset, np.float64)
        Jv, Jw = J[e, link, :3][:, cols], J[e, link, 3:][:, cols]
        out[e, :3] = Jv - skew(x - c[e, link]) @ Jw
        out[e, 3:] = Jw
    return out


def quat_mul(a, b):
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])


def pose_error(m, root, dof, chain, goal_pos, goal_quat=None, desc=None, frames=None):
    """[N, 6] float64 for one chain; goal_pos [N, 3], goal_quat [N, 4] xyzw or None (err[3:6] = 0)."""
    link, dofs, offset = chain_spec(chain)
    o, q, c = frames or link_frames(m, root, dof, desc)
    n = o.shape[0]
    err = np.zeros((n, 6))
    for e in range(n):
        x = o[e, link] + quat_R(q[e, link]) @ np.asarray(offset, np.float64)
        err[e, :3] = (np.asarray(goal_pos[e], np.float64) - np.asarray(root[e, :3], np.float64)) - x
        if goal_quat is not None:
            g = np.asarray(goal_quat[e], np.float64)
            g = g / np.linalg.norm(g)
            ql = q[e, link] / np.linalg.norm(q[e, link])
            p = quat_mul(g, np.concatenate([-ql[:3], ql[3:]]))
            err[e, 3:] = p[:3] * (1.0 if p[3] >= 0.0 else -1.0)
    return err


def dls_step(J, err, damping, rows=6):
    """[N, nd]: J^T (J J^T + damping^2 I)^-1 err over the first ``rows`` rows."""
    n, _, nd = J.shape
    dq = np.zeros((n, nd))
    for e in range(n):
        Je = J[e, :rows]
        dq[e] = Je.T @ np.linalg.solve(Je @ Je.T + damping ** 2 * np.eye(rows), err[e, :rows])
    return dq


def ik_ref(m, root, dof, chains, goal_pos, goal_quat=None, damping=0.3, desc=None):
    """(dq [N, K, 8], err [N, K, 6]) float64, the outputs of tg_ik_dls; goal_pos
    [N, K, 3], goal_quat [N, K, 4] or None."""
    desc = desc or abi.ModelDesc(m)
    n, K = root.shape[0], len(chains)
    J = jacobian_ref(m, _at_origin(root), dof, desc)
    frames = link_frames(m, root, dof, desc)
    dq, err = np.zeros((n, K, MAX_DOFS)), np.zeros((n, K, 6))
    for k, ch in enumerate(chains):
        nd = len(chain_spec(ch)[1])
        Jk = point_jacobian(m, root, dof, ch, desc, J=J, frames=frames)
        gq = None if goal_quat is None else goal_quat[:, k]
        err[:, k] = pose_error(m, root, dof, ch, goal_pos[:, k], gq, desc, frames=frames)
        dq[:, k, :nd] = dls_step(Jk, err[:, k], damping, rows=3 if goal_quat is None else 6)
    return dq, err


def link_pose_goal(m, root, dof, chain, desc=None):
    """(pos [N, 3] float32 world, quat [N, 4] float32): the pose of the chain's controlled
    point at this state -- a reachable goal.  Positions in float64 before the cast."""
    link, dofs, offset = chain_spec(chain)
    o, q, c = link_frames(m, root, dof, desc)
    n = o.shape[0]
    pos = np.zeros((n, 3))
    for e in range(n):
        pos[e] = np.asarray(root[e, :3], np.float64) + o[e, link] + quat_R(q[e, link]) @ np.asarray(offset, np.float64)
    return pos.astype(np.float32), q[:, link].astype(np.float32)


def path_dofs(m, link):
    """the DOFs on the path root -> link, root first (from link_parent / link_dof alone)"""
    a = abi.model_arrays(m)
    out, k = [], int(link)
    while k >= 0:
        if a["link_dof"][k] >= 0:
            out.append(int(a["link_dof"][k]))
        k = int(a["link_parent"][k])
    return out[::-1]
