"""float64 reference for the contact force distribution inside friction cones
(tgsim.h tg_contact_qp), the header's definition written out in numpy.  It is
built from tests/id_ref.py (Kinematics, id_ref), tests/jacobian_ref.py and
tests/contact_id_ref.py (the contact points and their Jacobians) and shares no
code with the kernel: the kernel never forms G, keeps a 6 x 6 factor and applies
(G^T W G + P)^-1 through the matrix inversion lemma; this file forms the dense
G (6 x 3 J) and the dense (G^T W G + P) (3 J x 3 J) and solves with that.

    b      = id_ref(...)                                  (tau of tg_inverse_dynamics)
    p_kv   = o_l + R_l (offset_k + (+-hx_k, +-hy_k, 0))   v: (+,+), (+,-), (-,-), (-,+)
    G_kv   = [1; [p_kv - c_root]x],  W = diag(1, 1, 1, 1/l^2, 1/l^2, 1/l^2)
    P      = diag(reg / s_k + rho),  c = G^T W b[0:6]
    q = c + rho (z - u);  x = (G^T W G + P)^-1 q;  xh = relax x + (1 - relax) z
    z = proj_C(xh + u);  u = u + xh - z                   from z = u = 0, iters times
    wrench_k = (sum_v z_kv, sum_v (p_kv - p_k) x z_kv)
    tau    = b - sum_k Jp_k^T wrench_k
A contact with s_k <= 0 is left out of the problem and gets exact zeros; an env
with every s_k <= 0 gets tau = b.  The dense matrix is inverted once per env and
applied per iteration, so that ``contact_qp_converged`` (the same iteration run
20 000 times) stays quick; with ``dtype=np.float32`` the iteration itself runs in
float32 (what float32 rounding alone does to the result)."""
from __future__ import annotations

import numpy as np

from tests.contact_id_ref import contact_points, point_jacobians, skew
from tests.id_ref import Kinematics, id_ref
from tests.jacobian_ref import quat_R
from tests.oracle_lib import rigid_body_states

DEFAULTS = dict(reg=0.03, rho=0.6, relax=1.6, iters=64)
CONVERGED_ITERS = 20000
SIGNS = ((1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0))


def patch_vertices(k: Kinematics, contacts, extents):
    """(p [N, K, 3], pv [N, K, 4, 3]) float64 relative to the root origin."""
    rb = rigid_body_states(k.desc, k.root0, k.dof).astype(np.float64)
    p = contact_points(k, contacts)
    pv = np.zeros((k.n, len(contacts), 4, 3))
    for e in range(k.n):
        for i, ((l, off), (hx, hy)) in enumerate(zip(contacts, extents)):
            R = quat_R(rb[e, l, 3:7])
            for v, (sx, sy) in enumerate(SIGNS):
                pv[e, i, v] = k.o[e, l] + R @ (np.asarray(off, np.float64) + np.array([sx * hx, sy * hy, 0.0]))
    return p, pv


def unit_normals(normals, n, K):
    """[N, K, 3] float64: normalised; a non-finite entry or a vector shorter than 1e-6 gives world z; None: world z."""
    out = np.zeros((n, K, 3))
    out[..., 2] = 1.0
    if normals is None:
        return out
    nn = np.asarray(normals, np.float64)
    for e in range(n):
        for i in range(K):
            v = nn[e, i]
            if np.isfinite(v).all() and np.linalg.norm(v) >= 1e-6:
                out[e, i] = v / np.linalg.norm(v)
    return out


def friction_of(mu, friction, n, K):
    """[N, K] float64: the tensor, or the scalar; negative and NaN as 0, above 1e6 as 1e6."""
    f = np.full((n, K), float(mu)) if friction is None else np.asarray(friction, np.float64).copy()
    f[~(f > 0)] = 0.0
    return np.minimum(f, 1e6)


def project_cone(w, nrm, mu):
    """The closed-form projection of the rows of w [J, 3] on the cones of normals nrm [J, 3] and coefficients mu [J]."""
    wn = (w * nrm).sum(-1)
    t = w - wn[:, None] * nrm
    tn = np.sqrt((t * t).sum(-1))
    inside = (wn >= 0) & (tn <= mu * wn)
    polar = ~inside & (mu * tn <= -wn)
    a = (mu * tn + wn) / (1 + mu * mu)
    safe = np.where(tn > 0, tn, 1).astype(w.dtype)
    edge = a[:, None] * (nrm + (mu / safe)[:, None] * t)
    z = np.where(inside[:, None], w, edge)
    z[polar] = 0
    return z


class Problem:
    """One env's dense problem: G [6, 3 J], W, P, c, the cones, over the vertices of the contacts with s_k > 0."""

    def __init__(self, b6, c_root, pv, nrm, mu, s, moment_arm, reg, rho):
        self.on = [i for i in range(len(s)) if s[i] > 0]
        J = 4 * len(self.on)
        self.G = np.zeros((6, 3 * J))
        self.nrm, self.mu, pdiag = np.zeros((J, 3)), np.zeros(J), np.zeros(3 * J)
        for a, i in enumerate(self.on):
            for v in range(4):
                j = 4 * a + v
                self.G[:3, 3 * j:3 * j + 3] = np.eye(3)
                self.G[3:, 3 * j:3 * j + 3] = skew(pv[i, v] - c_root)
                self.nrm[j], self.mu[j] = nrm[i], mu[i]
                pdiag[3 * j:3 * j + 3] = reg / s[i] + rho
        self.W = np.diag([1.0, 1.0, 1.0] + [1.0 / float(moment_arm) ** 2] * 3)
        self.b6, self.reg_w, self.rho = np.asarray(b6, np.float64), pdiag - rho, rho
        self.H = self.G.T @ self.W @ self.G + np.diag(pdiag)
        self.c = self.G.T @ self.W @ self.b6

    def objective(self, f):
        """1/2 |b6 - G f|^2_W + 1/2 reg sum_k (1 / s_k) sum_v |f_kv|^2 at f [J, 3] (or [3 J])."""
        f = np.asarray(f, np.float64).reshape(-1)
        d = self.b6 - self.G @ f
        return 0.5 * d @ self.W @ d + 0.5 * (self.reg_w * f * f).sum()

    def feasible(self, f, tol=0.0):
        f = np.asarray(f, np.float64).reshape(-1, 3)
        fn = (f * self.nrm).sum(-1)
        ft = np.linalg.norm(f - fn[:, None] * self.nrm, axis=-1)
        return bool((fn >= -tol).all() and (ft <= self.mu * fn + tol).all())

    def iterate(self, relax, iters, dtype=np.float64, trace=None):
        """(z [J, 3], max |x - z| of the last iteration); trace: a list that gets a copy of z per iteration."""
        J = len(self.mu)
        Hinv = np.linalg.inv(self.H).astype(dtype)
        c, nrm, mu = self.c.astype(dtype), self.nrm.astype(dtype), self.mu.astype(dtype)
        rho, relax = dtype(self.rho), dtype(relax)
        z, u, res = np.zeros((J, 3), dtype), np.zeros((J, 3), dtype), 0.0
        for _ in range(iters):
            x = (Hinv @ (c + rho * (z - u).reshape(-1))).reshape(J, 3)
            xh = relax * x + (dtype(1) - relax) * z
            zn = project_cone(xh + u, nrm, mu)
            un = u + xh - zn
            res = float(np.abs(x - zn).max()) if J else 0.0
            # at rest to 1e-15 of the largest force: further iterations move nothing that float64 resolves
            still = iters == CONVERGED_ITERS and max(np.abs(zn - z).max(), np.abs(un - u).max()) <= 1e-15 * np.abs(zn).max()
            z, u = zn, un
            if trace is not None:
                trace.append(z.copy())
            if still:
                break
        return z, res


def contact_qp_ref(m, root, dof, contacts, extents, mu=0.7, friction=None, normals=None, share=None, moment_arm=0.1,
                   reg=DEFAULTS["reg"], rho=DEFAULTS["rho"], relax=DEFAULTS["relax"], iters=DEFAULTS["iters"],
                   accel=None, gravity=True, velocity=True, g=(0.0, 0.0, -9.81), mass_scale=None, armature=None,
                   desc=None, kin=None, dtype=np.float64, problems=None):
    """dict(tau [N, 6 + D], wrench [N, K, 6], forces [N, K, 4, 3], info [N, 4], b [N, 6 + D]) float64; ``problems``:
    a list that gets each env's Problem (None for an env with every share 0)."""
    k = kin or Kinematics(m, root, dof, desc)
    n, K = k.n, len(contacts)
    b = id_ref(m, root, dof, accel=accel, gravity=gravity, velocity=velocity, g=g, mass_scale=mass_scale,
               armature=armature, kin=k)
    p, pv = patch_vertices(k, contacts, extents)
    Jp = point_jacobians(k, contacts, p)
    s = np.ones((n, K)) if share is None else np.asarray(share, np.float64).copy()
    s[~(s > 0)] = 0.0
    nrm, fr = unit_normals(normals, n, K), friction_of(mu, friction, n, K)
    tau, lam, f, info = b.copy(), np.zeros((n, K, 6)), np.zeros((n, K, 4, 3)), np.zeros((n, 4))
    for e in range(n):
        pr = None
        if (s[e] > 0).any():
            pr = Problem(b[e, :6], k.c[e, 0], pv[e], nrm[e], fr[e], s[e], moment_arm, reg, rho)
            z, res = pr.iterate(relax, iters, dtype)
            z = z.astype(np.float64)
            for a, i in enumerate(pr.on):
                f[e, i] = z[4 * a:4 * a + 4]
                lam[e, i, :3] = f[e, i].sum(0)
                lam[e, i, 3:] = np.cross(pv[e, i] - p[e, i], f[e, i]).sum(0)
                tau[e] -= Jp[e, i].T @ lam[e, i]
            info[e, 2] = res
            info[e, 3] = float(((f[e] * nrm[e][:, None, :]).sum(-1) > 0).sum())
        info[e, 0], info[e, 1] = np.linalg.norm(tau[e, :3]), np.linalg.norm(tau[e, 3:6])
        if problems is not None:
            problems.append(pr)
    return dict(tau=tau, wrench=lam, forces=f, info=info, b=b)


def contact_qp_converged(*args, **kw):
    """``contact_qp_ref`` with the same iteration run CONVERGED_ITERS times (or until it rests to 1e-15 of the largest force)."""
    kw["iters"] = CONVERGED_ITERS
    return contact_qp_ref(*args, **kw)
