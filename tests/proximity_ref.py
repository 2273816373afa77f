"""Float64 reference of the capsule proximity (tgsim.h tg_proximity), pinned by
tests/test_proximity_reference.py, and the scenarios of tests/test_gpu_proximity.py.

Distance of two segments.  The squared distance is a convex quadratic of (s, t)
on the unit square, so its minimum is the interior stationary point where that
lies in the open square, and otherwise on the border -- where one parameter is
0 or 1, the distance from an end point to the other segment.  ``segments``
takes the minimum over the four end-point-to-segment distances and the interior
solution where it is valid, and never branches on which case "should" apply.

Capsules are (link, p0, p1, radius) tuples here; the axis end points come from
tests/height_scan_ref.frame_poses, the forward kinematics the height scan and
the ray cast are checked against.

Exclusions (conditions, not measurements; the caps are asserted from the
reference alone in tests/test_proximity_reference.py):
  dist     a pair whose reference axis distance is under AXIS_MIN = 5 mm: the
           square root amplifies fp32 rounding there.  At most DIST_CAP = 2 %
           of a case's pairs.
  witness  a pair whose Hessian of the squared distance over the unclamped
           parameters, 2 [[a, -b], [-b, e]] (a, e the squared axis lengths, b
           the axes' dot product), has a smallest eigenvalue under HESS_MIN =
           1e-3 of the largest squared axis length: the minimiser slides along
           near-parallel axes.  A zero-length axis has no parameter: its row
           and column leave the Hessian (a sphere against a capsule: 2 e, never
           excluded; two spheres: nothing to exclude).  At most WITNESS_CAP =
           5 % of a case's pairs.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from tests import physics_models as pm
from tests.height_scan_ref import frame_poses

AXIS_MIN = 5e-3
HESS_MIN = 1e-3
DIST_CAP, WITNESS_CAP = 0.02, 0.05
ZERO2 = 1e-24          # squared length under which a float64 axis is a point (the inputs are fp32: exact zeros)

Prox = namedtuple("Prox", ["dist", "witness", "summary", "axis", "keep_dist", "keep_witness", "gap2", "near_margin"])


def point_segment(x, p, d):
    """(squared distance, parameter) of point x to the segment p + u d, u in [0, 1]."""
    dd = float(d @ d)
    u = 0.0 if dd <= ZERO2 else min(max(float((x - p) @ d) / dd, 0.0), 1.0)
    v = x - (p + u * d)
    return float(v @ v), u


def segments(p1, q1, p2, q2):
    """(delta, s, t): the least distance of the segments p1 q1 and p2 q2 and a minimiser."""
    p1, q1, p2, q2 = (np.asarray(v, np.float64) for v in (p1, q1, p2, q2))
    d1, d2 = q1 - p1, q2 - p2
    cand = []
    for s in (0.0, 1.0):
        f, t = point_segment(p1 + s * d1, p2, d2)
        cand.append((f, s, t))
    for t in (0.0, 1.0):
        f, s = point_segment(p2 + t * d2, p1, d1)
        cand.append((f, s, t))
    a, e, b = float(d1 @ d1), float(d2 @ d2), float(d1 @ d2)
    det = a * e - b * b
    if a > ZERO2 and e > ZERO2 and det > 1e-14 * a * e:
        r = p1 - p2
        c, f = float(d1 @ r), float(d2 @ r)
        s, t = (b * f - c * e) / det, (a * f - b * c) / det
        if 0.0 < s < 1.0 and 0.0 < t < 1.0:
            v = r + s * d1 - t * d2
            cand.append((float(v @ v), s, t))
    f, s, t = min(cand, key=lambda x: x[0])
    return float(np.sqrt(f)), s, t


def hessian_ok(d1, d2):
    """The witness condition of the module docstring for the axes d1, d2."""
    a, e, b = float(d1 @ d1), float(d2 @ d2), float(d1 @ d2)
    if a <= ZERO2 or e <= ZERO2:
        return True          # one parameter at the most: 2 e (or 2 a) against 1e-3 of the same squared length
    lam = 0.5 * ((a + e) - np.sqrt((a - e) ** 2 + 4.0 * b * b))
    return 2.0 * lam >= HESS_MIN * max(a, e)


def brute(p1, q1, p2, q2, n=201, rounds=4):
    """A dense grid over (s, t), refined ``rounds`` times about its best cell: the distance without any formula."""
    p1, q1, p2, q2 = (np.asarray(v, np.float64) for v in (p1, q1, p2, q2))
    lo, hi = np.zeros(2), np.ones(2)
    best = np.inf
    for _ in range(rounds):
        s = np.linspace(lo[0], hi[0], n)[:, None, None]
        t = np.linspace(lo[1], hi[1], n)[None, :, None]
        v = (p1 + s * (q1 - p1)) - (p2 + t * (q2 - p2))
        f = (v * v).sum(-1)
        i, j = np.unravel_index(int(np.argmin(f)), f.shape)
        best = min(best, float(f[i, j]))
        w = (hi - lo) / (n - 1)
        c = np.array([s[i, 0, 0], t[0, j, 0]])
        lo, hi = np.maximum(c - w, 0.0), np.minimum(c + w, 1.0)
    return float(np.sqrt(best))


def proximity_points(p0, p1, radius, pairs, margin):
    """The outputs for one env from the world end points p0, p1 [C, 3] and the radii [C]."""
    P = len(pairs)
    dist, wit, axis = np.zeros(P), np.zeros((P, 6)), np.zeros(P)
    kd, kw = np.ones(P, bool), np.ones(P, bool)
    for k, (ia, ib) in enumerate(pairs):
        delta, s, t = segments(p0[ia], p1[ia], p0[ib], p1[ib])
        axis[k] = delta
        dist[k] = delta - radius[ia] - radius[ib]
        wit[k, :3] = p0[ia] + s * (p1[ia] - p0[ia])
        wit[k, 3:] = p0[ib] + t * (p1[ib] - p0[ib])
        kd[k] = delta >= AXIS_MIN
        kw[k] = hessian_ok(p1[ia] - p0[ia], p1[ib] - p0[ib])
    first = int(np.argmin(dist))
    summary = np.array([dist[first], first, (dist < margin).sum(), np.maximum(margin - dist, 0.0).sum()])
    two = np.sort(dist)[:2]
    gap2 = float(two[1] - two[0]) if P > 1 else np.inf
    return dist, wit, summary, axis, kd, kw, gap2, float(np.abs(dist - margin).min())


def proximity_ref(m, root, dof, capsules, pairs, margin):
    """Prox of float64 arrays: dist [N, P], witness [N, P, 6], summary [N, 4], axis [N, P] (the axis distance
    delta), keep_dist / keep_witness [N, P] (the module's exclusions), gap2 [N] (the difference of the two smallest
    dist) and near_margin [N] (the least |dist - margin|)."""
    root = np.asarray(root, np.float32)
    frames = [(int(l), tuple(p0)) for l, p0, _p1, _r in capsules] + [(int(l), tuple(p1)) for l, _p0, p1, _r in capsules]
    p, _R = frame_poses(m, root, dof, frames)
    Cn = len(capsules)
    radius = np.array([float(np.float32(r)) for _l, _p0, _p1, r in capsules])
    rows = [proximity_points(p[e, :Cn], p[e, Cn:], radius, pairs, margin) for e in range(root.shape[0])]
    return Prox(*(np.array([r[k] for r in rows]) for k in range(8)))


def capsule_tuples(capsules):
    """tg_capsule structs as the (link, p0, p1, radius) tuples of this module (fp32 values, exactly)."""
    return [(int(c.link), tuple(float(v) for v in c.p0), tuple(float(v) for v in c.p1), float(c.radius))
            for c in capsules]


def as_structs(capsules):
    from thormang_isaacgym_amd.sim import make_capsule
    return [make_capsule(l, p0, p1, r) for l, p0, p1, r in capsules]


# ------------------------------------------------------------------ known answers
# (capsule a, capsule b, delta): end points in one frame, radii 0.03 and 0.05
_A = 0.25   # exactly representable lengths
KNOWN = [
    ("two spheres", ((0, 0, 0), (0, 0, 0)), ((0.5, 0, 0), (0.5, 0, 0)), 0.5),
    ("crossed perpendicular", ((-_A, 0, 0), (_A, 0, 0)), ((0, -_A, 0.125), (0, _A, 0.125)), 0.125),
    ("end to end", ((0, 0, 0), (_A, 0, 0)), ((0.5, 0, 0), (0.5, 0.5, 0)), 0.25),
    ("end to interior", ((0, 0.125, 0), (0, 0.5, 0)), ((-_A, 0, 0), (_A, 0, 0)), 0.125),
    ("parallel overlapping", ((0, 0, 0), (0.5, 0, 0)), ((0.25, 0.125, 0), (0.75, 0.125, 0)), 0.125),
    ("parallel apart", ((0, 0, 0), (0.25, 0, 0)), ((0.5, 0.375, 0), (1.0, 0.375, 0)), float(np.hypot(0.25, 0.375))),
    ("parallel opposed", ((0, 0, 0), (0.5, 0, 0)), ((0.75, 0.125, 0), (0.25, 0.125, 0)), 0.125),
    ("collinear apart", ((0, 0, 0), (0.25, 0, 0)), ((0.5, 0, 0), (1.0, 0, 0)), 0.25),
    ("collinear overlapping", ((0, 0, 0), (0.5, 0, 0)), ((0.25, 0, 0), (1.0, 0, 0)), 0.0),
    ("both degenerate", ((0, 0.25, 0), (0, 0.25, 0)), ((0, 0, 0.25), (0, 0, 0.25)), float(np.hypot(0.25, 0.25))),
    ("sphere to interior", ((0.125, 0.25, 0), (0.125, 0.25, 0)), ((0, 0, 0), (0.5, 0, 0)), 0.25),
    ("capsule to sphere end", ((0, 0, 0), (0.5, 0, 0)), ((0.75, 0, 0), (0.75, 0, 0)), 0.25),
    ("crossing axes", ((-_A, 0, 0), (_A, 0, 0)), ((0, -_A, 0), (0, _A, 0)), 0.0),
    ("skew interior", ((0, 0, 0), (1, 0, 0)), ((0.5, -0.5, 0.25), (0.5, 0.5, 0.5)), float(0.375 / np.hypot(1.0, 0.25))),
    ("t clamped then s", ((0, 0, 0), (1, 0, 0)), ((1.5, 0.25, 0), (2.5, 1.0, 0)), float(np.hypot(0.5, 0.25))),
    ("near parallel", ((0, 0, 0), (0.5, 0, 0)), ((0, 0.125, 0), (0.5, 0.125 + 2.0 ** -12, 0)), 0.125),
]
KNOWN_RADII = (0.03, 0.05)
assert len(KNOWN) == 16


def known_capsules(link=0):
    """The 32 capsules and 16 pairs of KNOWN on one link, and dist = delta - 0.03 - 0.05 as fp32 rounds the radii."""
    caps, pairs, want = [], [], []
    ra, rb = (float(np.float32(r)) for r in KNOWN_RADII)
    for k, (_name, a, b, delta) in enumerate(KNOWN):
        caps += [(link, tuple(map(float, a[0])), tuple(map(float, a[1])), ra),
                 (link, tuple(map(float, b[0])), tuple(map(float, b[1])), rb)]
        pairs.append((2 * k, 2 * k + 1))
        want.append(delta - ra - rb)
    return caps, pairs, np.array(want)


# ------------------------------------------------------------------ scenarios of the GPU test
N = 5
FAR = (40.07, 30.11, 0.0)     # env 1: env 0's pose, this far away
CASES = ["thormang", "gogoro", "jit_walker", "kat_free"]
MARGIN = 0.02
CROSSED_ENV = 2               # thormang: the env with crossed legs


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return {"jit_walker": pm.jit_walker, "kat_free": pm.free_body}.get(name, lambda: load_model(name))()


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def case_capsules(case, m):
    """(capsules as tuples, pairs) of a case."""
    from thormang_isaacgym_amd.sim import capsule_pairs, limb_capsule, link_tree, make_capsule
    parent, origin = link_tree(m)
    if case == "thormang":
        from thormang_isaacgym_amd.tasks.thormang_walk import walk_self_capsules
        caps = walk_self_capsules(m)
        return capsule_tuples(caps), capsule_pairs(parent, caps)
    if case == "gogoro":
        li = m.link_index
        limbs = [limb_capsule(parent, origin, li(s + "_arm_el_y_link"), li(s + "_arm_wr_r_link"), 0.045)
                 for s in "lr"]
        hands = [limb_capsule(parent, origin, li(s + "_arm_wr_p_link"), li(s + "_arm_end_link"), 0.04) for s in "lr"]
        frame = [make_capsule(li("head"), (0.0, 0.0, -0.2), (0.0, 0.0, 0.3), 0.05),
                 make_capsule(li("body"), (-0.4, 0.0, 0.1), (0.3, 0.0, 0.1), 0.12)]
        caps = limbs + hands + frame
        return capsule_tuples(caps), [(a, b) for a in range(4) for b in (4, 5)]
    if case == "jit_walker":
        li = m.link_index
        caps = [make_capsule(li("torso"), (0.0, -0.1, 0.0), (0.0, 0.1, 0.0), 0.1)]
        for s in "lr":
            caps += [make_capsule(li(s + "_thigh"), (0, 0, 0), (0, 0, -0.3), 0.05),
                     make_capsule(li(s + "_shin"), (0, 0, 0), (0, 0, -0.26), 0.04)]
        return capsule_tuples(caps), capsule_pairs(parent, caps, min_hops=2)
    caps, pairs, _want = known_capsules()               # kat_free: one link, every distance a known constant
    return caps, pairs


@functools.lru_cache(maxsize=None)
def scenario(case, n=N, seed=12):
    """(model, capsules, pairs, root, dof) of a case; no GPU needed."""
    m = _model(case)
    rs = np.random.default_rng(seed)
    caps, pairs = case_capsules(case, m)
    D = m.num_dof
    root = np.zeros((n, 13), np.float32)
    dof = np.zeros((n, D, 2), np.float32)
    dof[..., 0] = rs.uniform(-0.4, 0.4, (n, D))
    xyz = np.stack([rs.uniform(-4.0, 30.0, n), rs.uniform(-2.0, 30.0, n), rs.uniform(0.8, 1.2, n)], 1)
    yaw = rs.uniform(-np.pi, np.pi, n)
    for e in range(n):
        ax, ang = rs.uniform(0, 2 * np.pi), rs.uniform(0.05, 0.15)
        tilt = np.array([np.cos(ax) * np.sin(ang / 2), np.sin(ax) * np.sin(ang / 2), 0.0, np.cos(ang / 2)])
        q = _quat_mul(np.array([0.0, 0.0, np.sin(yaw[e] / 2), np.cos(yaw[e] / 2)]), tilt)
        root[e, :3], root[e, 3:7] = xyz[e], q / np.linalg.norm(q)
    if n > 1:
        root[1], dof[1] = root[0], dof[0]
        root[1, :3] = root[0, :3] + np.asarray(FAR, np.float32)
    if case == "thormang" and n > CROSSED_ENV:
        dni = m.dof_name_to_id()
        dof[CROSSED_ENV, :, 0] = 0.0
        for name, v in (("l_leg_hip_r", 0.45), ("r_leg_hip_r", -0.45), ("l_leg_hip_p", -0.3), ("l_leg_kn_p", 0.6),
                        ("r_leg_hip_p", 0.25), ("r_leg_kn_p", -0.55)):
            dof[CROSSED_ENV, dni[name], 0] = v
    return m, tuple(caps), tuple(pairs), root, dof.reshape(n * D, 2)


@functools.lru_cache(maxsize=None)
def reference(case, n=N, seed=12, margin=MARGIN):
    m, caps, pairs, root, dof = scenario(case, n, seed)
    return proximity_ref(m, root, dof, list(caps), list(pairs), margin)


def cycled_pairs(caps, parent, count):
    """``count`` pairs of the capsules: every pair of capsules on different links, in order, then again with the two
    swapped, cycled up to ``count`` -- the shapes P = 1, 63, 64, 65, 256 of the GPU test."""
    from thormang_isaacgym_amd.sim import link_hops
    base = [(a, b) for a in range(len(caps)) for b in range(a + 1, len(caps))
            if link_hops(parent, caps[a][0], caps[b][0]) >= 3]
    both = base + [(b, a) for a, b in base]
    return [both[k % len(both)] for k in range(count)]


def default_stance(m, cfg_angles):
    """(root, dof) of one env at the walk's default stance."""
    root = np.zeros((1, 13), np.float32)
    root[0, 2], root[0, 6] = 0.79, 1.0
    dof = np.zeros((m.num_dof, 2), np.float32)
    dni = m.dof_name_to_id()
    for name, v in cfg_angles.items():
        dof[dni[name], 0] = v
    return root, dof
