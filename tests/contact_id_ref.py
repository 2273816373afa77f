"""float64 reference for the contact-consistent inverse dynamics (tgsim.h
tg_contact_inverse_dynamics), the header's definition written out in numpy.  It
is built only from tests/id_ref.py (Kinematics, id_ref) and tests/jacobian_ref.py
and shares no code with the kernel: the kernel takes its moments about the
share-weighted mean contact point and solves a 3 x 3 system, this file forms the
6 x 6 matrix of the header about the root link's centre of mass.

    b      = id_ref(...)                                  (tau of tg_inverse_dynamics)
    p_k    = o_l + R_l offset_k
    Jp_k   = (Jv_l - [p_k - c_l]x Jw_l ; Jw_l)            from jacobian_ref's rows
    G_k    = Jp_k[:, 0:6]^T
    A      = sum_k s_k G_k Dm G_k^T,  Dm = diag(1, 1, 1, l^2, l^2, l^2)
    y      = A^-1 b[0:6]
    lam_k  = s_k Dm G_k^T y                               (= (s_k (y_f + y_n x r_k), s_k l^2 y_n))
    tau    = b - sum_k Jp_k^T lam_k
Negative shares count as 0; a contact with s_k = 0 gets an exactly zero wrench
and drops out of every sum; an env with every s_k = 0 gets tau = b."""
from __future__ import annotations

import numpy as np

from tests.id_ref import Kinematics, id_ref
from tests.jacobian_ref import quat_R
from tests.oracle_lib import rigid_body_states


def skew(v):
    x, y, z = (float(a) for a in v)
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def contact_points(k: Kinematics, contacts):
    """p [N, K, 3] float64 relative to the root origin; contacts = [(link, (ox, oy, oz)), ...]."""
    rb = rigid_body_states(k.desc, k.root0, k.dof).astype(np.float64)
    p = np.zeros((k.n, len(contacts), 3))
    for e in range(k.n):
        for i, (l, off) in enumerate(contacts):
            p[e, i] = k.o[e, l] + quat_R(rb[e, l, 3:7]) @ np.asarray(off, np.float64)
    return p


def point_jacobians(k: Kinematics, contacts, p=None):
    """Jp [N, K, 6, 6 + D]: the linear velocity of p_k and the angular velocity of its link per unit u."""
    p = contact_points(k, contacts) if p is None else p
    Jp = np.zeros((k.n, len(contacts), 6, 6 + k.D))
    for e in range(k.n):
        for i, (l, _off) in enumerate(contacts):
            Jv, Jw = k.J[e, l, :3], k.J[e, l, 3:]
            Jp[e, i, :3] = Jv - skew(p[e, i] - k.c[e, l]) @ Jw
            Jp[e, i, 3:] = Jw
    return Jp


def wrench_cost(lam, share, moment_arm):
    """sum_k (|f_k|^2 + |n_k|^2 / l^2) / s_k per env, over the contacts with s_k > 0; lam [N, K, 6]."""
    s = np.maximum(np.asarray(share, np.float64), 0.0)
    c = (lam[..., :3] ** 2).sum(-1) + (lam[..., 3:] ** 2).sum(-1) / moment_arm ** 2
    return np.where(s > 0, c / np.where(s > 0, s, 1.0), 0.0).sum(-1)


def contact_id_ref(m, root, dof, contacts, share=None, moment_arm=0.1, accel=None, gravity=True, velocity=True,
                   g=(0.0, 0.0, -9.81), mass_scale=None, armature=None, desc=None, kin=None, parts=False):
    """(tau [N, 6 + D], wrench [N, K, 6]) float64; with ``parts`` also (b, Jp)."""
    k = kin or Kinematics(m, root, dof, desc)
    n, K = k.n, len(contacts)
    b = id_ref(m, root, dof, accel=accel, gravity=gravity, velocity=velocity, g=g, mass_scale=mass_scale,
               armature=armature, kin=k)
    Jp = point_jacobians(k, contacts)
    s = np.ones((n, K)) if share is None else np.maximum(np.asarray(share, np.float64), 0.0)
    Dm = np.diag([1.0, 1.0, 1.0] + [float(moment_arm) ** 2] * 3)
    tau, lam = b.copy(), np.zeros((n, K, 6))
    for e in range(n):
        on = [i for i in range(K) if s[e, i] > 0]
        if not on:
            continue
        G = {i: Jp[e, i, :, :6].T for i in on}
        A = sum(s[e, i] * G[i] @ Dm @ G[i].T for i in on)
        y = np.linalg.solve(A, b[e, :6])
        for i in on:
            lam[e, i] = s[e, i] * Dm @ G[i].T @ y
            tau[e] -= Jp[e, i].T @ lam[e, i]
    return (tau, lam, b, Jp) if parts else (tau, lam)
