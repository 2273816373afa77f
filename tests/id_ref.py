"""float64 reference for the inverse dynamics (tgsim.h tg_inverse_dynamics),
analytic and built only from the CPU oracle's link states and
tests/jacobian_ref.py -- it shares no code with the kernels.

With u = (root com velocity, root angular velocity, qd), J[e, l] = (Jv, Jw),
R_l I_l R_l^T and H of jacobian_ref / mass_matrix_ref, s the body mass scales
and g the gravity vector:
    tau = H a + sum_l s_l [ Jv_l^T m_l (ab_l - [gravity] g)
                            + Jw_l^T (R_l I_l R_l^T alb_l + w_l x (R_l I_l R_l^T w_l)) ]
w_l = Jw_l u; ab_l and alb_l, the velocity-product accelerations of link l's
com and of its rotation (d/dt of Jv_l u and Jw_l u with u' = 0), come from the
standard outward recursion over link_parent / link_dof, on the oracle's link
origins o_l and coms c_l and the joint axes read off the Jacobian's own column:
    root:       alb = 0, ao = -w x (w x (c - o))            (its COM does not accelerate)
    revolute:   alb = alb_p + w_p x a qd,  ao = ao_p + alb_p x r + w_p x (w_p x r)
    prismatic:  alb = alb_p,               ao = ao_p + alb_p x r + w_p x (w_p x r) + 2 w_p x a qd
    fixed:      as revolute with qd = 0
    ab = ao + alb x (c - o) + w x (w x (c - o)),   r = o - o_p
Without ``velocity`` u is taken as 0.  The float32 state and property arrays
are taken as given; everything after the oracle is float64, and the oracle is
evaluated with the root link at the origin (no absolute position enters)."""
from __future__ import annotations

import numpy as np

from tests.jacobian_ref import jacobian_ref, link_inertias_world, mass_matrix_ref, quat_R
from tests.oracle_lib import rigid_body_states
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.model.urdf import JOINT_PRISMATIC, JOINT_REVOLUTE

GRAVITY = (0.0, 0.0, -9.81)


def _at_origin(root):
    r = np.array(root, np.float32)
    r[:, :3] = 0.0
    return r


def generalised_velocity(m, root, dof):
    """u [N, 6 + D] float64"""
    n, D = root.shape[0], m.num_dof
    return np.concatenate([np.asarray(root, np.float64)[:, 7:13],
                           np.asarray(dof, np.float64).reshape(n, D, 2)[:, :, 1]], axis=1)


class Kinematics:
    """What the reference needs at one state: J, R I R^T, link origins and coms
    (relative to the root origin), all float64."""

    def __init__(self, m, root, dof, desc=None):
        self.m, self.desc = m, desc or abi.ModelDesc(m)
        r0 = _at_origin(root)
        self.root0, self.dof = r0, np.asarray(dof, np.float32)
        self.n, self.L, self.D = root.shape[0], m.num_bodies, m.num_dof
        self.J = jacobian_ref(m, r0, dof, self.desc)
        self.Iw = link_inertias_world(m, r0, dof, self.desc)
        rb = rigid_body_states(self.desc, r0, self.dof).astype(np.float64)
        arr = abi.model_arrays(m)
        self.li = np.asarray(arr["link_inertia"], np.float64)
        self.parent = [int(x) for x in arr["link_parent"]]
        self.ldof = [int(x) for x in arr["link_dof"]]
        self.jtype = [int(x) for x in arr["link_jtype"]]
        self.o = rb[:, :, :3]
        self.c = np.zeros((self.n, self.L, 3))
        for e in range(self.n):
            for l in range(self.L):
                self.c[e, l] = self.o[e, l] + quat_R(rb[e, l, 3:7]) @ self.li[l, 1:4]


def velocity_product_accelerations(k: Kinematics, u):
    """(ab [N, L, 3], alb [N, L, 3], w [N, L, 3]) float64 at the generalised velocity u [N, 6 + D]."""
    n, L = k.n, k.L
    ab, alb, ao, w = (np.zeros((n, L, 3)) for _ in range(4))
    for e in range(n):
        for l in range(L):                                   # (parents come before their children)
            w[e, l] = k.J[e, l, 3:] @ u[e]
            p = k.parent[l]
            rc = k.c[e, l] - k.o[e, l]
            if p < 0:
                ao[e, l] = -np.cross(w[e, l], np.cross(w[e, l], rc))
            else:
                assert p < l
                r = k.o[e, l] - k.o[e, p]
                wp = w[e, p]
                ao[e, l] = ao[e, p] + np.cross(alb[e, p], r) + np.cross(wp, np.cross(wp, r))
                alb[e, l] = alb[e, p]
                d = k.ldof[l]
                if d >= 0 and k.jtype[l] == JOINT_REVOLUTE:
                    alb[e, l] += np.cross(wp, k.J[e, l, 3:, 6 + d] * u[e, 6 + d])
                elif d >= 0 and k.jtype[l] == JOINT_PRISMATIC:
                    ao[e, l] += 2.0 * np.cross(wp, k.J[e, l, :3, 6 + d] * u[e, 6 + d])
            ab[e, l] = ao[e, l] + np.cross(alb[e, l], rc) + np.cross(w[e, l], np.cross(w[e, l], rc))
    return ab, alb, w


def id_ref(m, root, dof, accel=None, gravity=True, velocity=True, g=GRAVITY, mass_scale=None, armature=None,
           desc=None, kin=None, parts=False):
    """tau [N, 6 + D] float64.  accel [N, 6 + D] or None, mass_scale [N, L] or
    None (ones), armature [N, D] or None (zeros), g the gravity vector.  With
    ``parts`` also (ab, alb, w, H)."""
    k = kin or Kinematics(m, root, dof, desc)
    n, L, D = k.n, k.L, k.D
    u = generalised_velocity(m, root, dof) if velocity else np.zeros((n, 6 + D))
    ab, alb, w = velocity_product_accelerations(k, u)
    s = np.ones((n, L)) if mass_scale is None else np.asarray(mass_scale, np.float64)
    gv = np.asarray(g, np.float64) if gravity else np.zeros(3)
    tau = np.zeros((n, 6 + D))
    for e in range(n):
        for l in range(L):
            Jv, Jw = k.J[e, l, :3], k.J[e, l, 3:]
            Iw = k.Iw[e, l]
            tau[e] += s[e, l] * (Jv.T @ (k.li[l, 0] * (ab[e, l] - gv))
                                 + Jw.T @ (Iw @ alb[e, l] + np.cross(w[e, l], Iw @ w[e, l])))
    H = None
    if accel is not None or parts:
        H = mass_matrix_ref(m, k.root0, dof, mass_scale=mass_scale, armature=armature, J=k.J, desc=k.desc)
    if accel is not None:
        tau += np.einsum("eij,ej->ei", H, np.asarray(accel, np.float64))
    return (tau, ab, alb, w, H) if parts else tau


def efforts_ref(tau, effort, base, dofs=None, accumulate=False):
    """[N, D]: ``base`` with clamp(tau[6 + d]) (clamp(base + tau[6 + d]) with
    ``accumulate``) to +-effort [N, D] at the selected DOFs (None: all)."""
    out = np.array(base, np.float64)
    D = out.shape[1]
    sel = list(range(D)) if dofs is None else list(dofs)
    eff = np.asarray(effort, np.float64)
    t = tau[:, 6:][:, sel] + (out[:, sel] if accumulate else 0.0)
    out[:, sel] = np.clip(t, -eff[:, sel], eff[:, sel])
    return out
