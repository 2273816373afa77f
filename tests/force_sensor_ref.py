"""float64 reference of the force sensor tensor (tgsim.h
tg_set_force_sensor_tensor): the wrench a link's contact rows exert, taken
about a sensor point.

A row j has a stored-velocity multiplier lam_j (an impulse, N s), a direction
d_j, a point of application x_j and a torsion flag: a torsion row carries the
pure moment lam_j d_j and no force.  Over a substep of length h

    f = (1 / h) sum_j lam_j d_j                           (non-torsion rows)
    n = (1 / h) sum_j lam_j ((x_j - p) x d_j + t_j)       (t_j = d_j on a torsion row, else 0)

in world axes; ``R`` (the link's rotation, link -> world) turns both into the
link's own axes, R^T f and R^T n."""
import numpy as np


def wrench_at(p, lam, d, x, torsion, h, R=None):
    """(f, n) [6] about the point ``p`` [3] from the rows ``lam`` [K], ``d``
    [K,3], ``x`` [K,3], ``torsion`` [K] (bool), substep ``h``; world axes, or
    the axes of ``R`` (link -> world) when given."""
    p = np.asarray(p, np.float64)
    lam = np.asarray(lam, np.float64)
    d = np.asarray(d, np.float64).reshape(-1, 3)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    tor = np.asarray(torsion, bool)
    f = np.zeros(3)
    n = np.zeros(3)
    for j in range(len(lam)):
        if tor[j]:
            n += lam[j] * d[j]
        else:
            f += lam[j] * d[j]
            n += lam[j] * np.cross(x[j] - p, d[j])
    w = np.concatenate([f, n]) / h
    if R is not None:
        R = np.asarray(R, np.float64)
        w = np.concatenate([R.T @ w[:3], R.T @ w[3:]])
    return w


def transport(w, p_from, p_to):
    """The wrench ``w`` = (f, n about p_from) taken about ``p_to`` instead
    (same axes): n' = n + (p_from - p_to) x f."""
    w = np.asarray(w, np.float64)
    return np.concatenate([w[:3], w[3:] + np.cross(np.asarray(p_from, np.float64) - np.asarray(p_to, np.float64),
                                                   w[:3])])


def torus_patch_rows(Rs, c, params):
    """Row geometry of a torus (a wheel: axis = the shape's z, ``params`` =
    major and minor radius) on flat ground: one normal row at the support
    point and two friction rows there, along the rolling direction axis x e_z
    and e_z x that.  Returns (pts [1,3], d [3,3], x [3,3], torsion [3])."""
    Rs, c = np.asarray(Rs, np.float64), np.asarray(c, np.float64)
    nn = np.array([0.0, 0.0, 1.0])
    ax = Rs[:, 2]
    dd = nn - (ax @ nn) * ax
    nd = np.linalg.norm(dd)
    if nd < 1e-6:
        dd, nd = np.array([1.0, 0.0, 0.0]), 1.0
    pt = c - (params[0] / nd) * dd - params[1] * nn
    t1 = np.cross(ax, nn)
    t1 = t1 / np.linalg.norm(t1) if np.linalg.norm(t1) > 1e-6 else np.array([1.0, 0.0, 0.0])
    t2 = np.cross(nn, t1)
    return pt[None, :], np.array([nn, t1, t2]), np.array([pt, pt, pt]), np.array([False] * 3)


def box_patch_rows(Rs, c, half, margin=None, phi=None):
    """Row geometry of a box patch on flat ground (normal e_z), as the solver
    builds it: ``Rs`` / ``c`` the box's world rotation and centre, ``half`` its
    half extents.  Returns (pts [4,3] the support face's corners in the
    solver's order, d [7,3], x [7,3], torsion [7]): four normal rows at the
    corners, two friction rows along t1 = e_x, t2 = e_y and the torsion row
    about e_z, all three anchored at the centroid of the corners weighted by
    clamp((margin - phi_k) / margin, 0, 1) (``phi``: the corners' separations,
    default their heights; all weights 0: the plain mean)."""
    Rs, c = np.asarray(Rs, np.float64), np.asarray(c, np.float64)
    nn = np.array([0.0, 0.0, 1.0])
    ex, ey, ez = Rs[:, 0], Rs[:, 1], Rs[:, 2]
    z = np.array([ex @ nn, ey @ nn, ez @ nn])
    a = np.abs(z)
    hx, hy, hz = half
    if a[2] >= a[0] and a[2] >= a[1]:
        fn, u1, u2 = (-hz if z[2] > 0 else hz) * ez, hx * ex, hy * ey
    elif a[1] >= a[0]:
        fn, u1, u2 = (-hy if z[1] > 0 else hy) * ey, hx * ex, hz * ez
    else:
        fn, u1, u2 = (-hx if z[0] > 0 else hx) * ex, hy * ey, hz * ez
    pts = np.array([c + fn - u1 - u2, c + fn + u1 - u2, c + fn - u1 + u2, c + fn + u1 + u2])
    phi = pts[:, 2] if phi is None else np.asarray(phi, np.float64)
    w = np.zeros(4) if margin is None else np.clip((margin - phi) / margin, 0.0, 1.0)
    cen = (w @ pts) / w.sum() if w.sum() > 0 else pts.mean(axis=0)
    t1, t2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    d = np.array([nn, nn, nn, nn, t1, t2, nn])
    x = np.array([pts[0], pts[1], pts[2], pts[3], cen, cen, cen])
    return pts, d, x, np.array([False] * 6 + [True])
