"""float64 reference for the centroidal quantities (tgsim.h tg_centroidal),
built only from the CPU oracle's link states and tests/jacobian_ref.py -- it
shares no code with the kernels -- and in two independent ways:

* ``state_ref``: directly from the oracle's link states
  (``oracle_lib.rigid_body_states``: link origins, orientations, com and
  angular velocities) and ``jacobian_ref.link_inertias_world``: with m'_l = s_l
  m_l, I'_l = s_l R_l I_l R_l^T, c_l and v_l the link coms and their
  velocities, w_l the angular velocities,
      M = sum m'_l,  c = sum m'_l c_l / M,  c' = sum m'_l v_l / M,
      k = sum (I'_l w_l + (c_l - c) x m'_l v_l),
      I_G = sum (I'_l + m'_l (|d|^2 1 - d d^T)),  d = c_l - c;
* ``matrix_ref``: A = sum_l [ m'_l Jv_l ; I'_l Jw_l + (c_l - c) x m'_l Jv_l ]
  from ``jacobian_ref`` (one oracle call per column), so that A u against the
  state compares the two routes.

``bias_ref`` is the momentum rate at u' = 0 without gravity from the velocity-
product accelerations of tests/id_ref.py:
    sum_l [ m'_l ab_l ; I'_l alb_l + w_l x I'_l w_l + (c_l - c) x m'_l ab_l ].

The float32 state arrays are taken as given; everything after the oracle is
float64.  The oracle is evaluated with the root link at the origin and the
root position is added to c last, so nothing but c depends on where the env
sits."""
from __future__ import annotations

import numpy as np

from tests.id_ref import Kinematics, generalised_velocity, velocity_product_accelerations
from tests.jacobian_ref import link_inertias_world, quat_R
from tests.oracle_lib import rigid_body_states
from thormang_isaacgym_amd import abi

STATE = abi.TG_CENTROIDAL_STATE   # floats per env of the state, the ABI's layout


def sym6(I):
    """xx yy zz xy xz yz of a symmetric 3 x 3"""
    return np.array([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])


def sym33(s):
    xx, yy, zz, xy, xz, yz = (float(v) for v in s)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def _scales(m, n, mass_scale):
    return np.ones((n, m.num_bodies)) if mass_scale is None else np.asarray(mass_scale, np.float64)


def state_ref(m, root, dof, mass_scale=None, desc=None):
    """state [N, 16] float64 from the oracle's link states."""
    desc = desc or abi.ModelDesc(m)
    n, L = root.shape[0], m.num_bodies
    r0 = np.array(root, np.float32)
    r0[:, :3] = 0.0
    dof = np.asarray(dof, np.float32)
    rb = rigid_body_states(desc, r0, dof).astype(np.float64)
    Iw = link_inertias_world(m, r0, dof, desc)
    li = np.asarray(abi.model_arrays(m)["link_inertia"], np.float64)
    s = _scales(m, n, mass_scale)
    out = np.zeros((n, STATE))
    for e in range(n):
        mp = s[e] * li[:, 0]
        cl = np.array([rb[e, l, :3] + quat_R(rb[e, l, 3:7]) @ li[l, 1:4] for l in range(L)])
        v, w = rb[e, :, 7:10], rb[e, :, 10:13]
        M = mp.sum()
        c = (mp[:, None] * cl).sum(axis=0) / M
        cd = (mp[:, None] * v).sum(axis=0) / M
        k, IG = np.zeros(3), np.zeros((3, 3))
        for l in range(L):
            d = cl[l] - c
            k += s[e, l] * Iw[e, l] @ w[l] + np.cross(d, mp[l] * v[l])
            IG += s[e, l] * Iw[e, l] + mp[l] * (d @ d * np.eye(3) - np.outer(d, d))
        out[e, 0:3] = c + np.asarray(root, np.float64)[e, :3]
        out[e, 3:6], out[e, 6:9], out[e, 9], out[e, 10:16] = cd, k, M, sym6(IG)
    return out


def com_relative(k: Kinematics, mass_scale=None):
    """(M [N], c [N, 3] relative to the root origin) from the link coms of a Kinematics."""
    s = _scales(k.m, k.n, mass_scale)
    mp = s * k.li[None, :, 0]
    M = mp.sum(axis=1)
    return M, (mp[:, :, None] * k.c).sum(axis=1) / M[:, None]


def matrix_ref(m, root, dof, mass_scale=None, kin=None):
    """A [N, 6, 6 + D] float64 by the header's definition, from jacobian_ref."""
    k = kin or Kinematics(m, root, dof)
    s = _scales(m, k.n, mass_scale)
    _M, c = com_relative(k, mass_scale)
    A = np.zeros((k.n, 6, 6 + k.D))
    for e in range(k.n):
        for l in range(k.L):
            mp = s[e, l] * k.li[l, 0]
            Jv, Jw = k.J[e, l, :3], k.J[e, l, 3:]
            A[e, :3] += mp * Jv
            A[e, 3:] += s[e, l] * k.Iw[e, l] @ Jw + np.cross(k.c[e, l] - c[e], mp * Jv, axisb=0, axisc=0)
    return A


def bias_ref(m, root, dof, mass_scale=None, kin=None):
    """A' u [N, 6] float64: the momentum rate at u' = 0, no gravity."""
    k = kin or Kinematics(m, root, dof)
    s = _scales(m, k.n, mass_scale)
    _M, c = com_relative(k, mass_scale)
    ab, alb, w = velocity_product_accelerations(k, generalised_velocity(m, root, dof))
    out = np.zeros((k.n, 6))
    for e in range(k.n):
        for l in range(k.L):
            f = s[e, l] * k.li[l, 0] * ab[e, l]
            Iw = s[e, l] * k.Iw[e, l]
            out[e, :3] += f
            out[e, 3:] += Iw @ alb[e, l] + np.cross(w[e, l], Iw @ w[e, l]) + np.cross(k.c[e, l] - c[e], f)
    return out
