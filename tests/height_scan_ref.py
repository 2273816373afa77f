"""float64 reference for the height scan (tgsim.h tg_height_scan), a plain numpy
restatement of the header's definitions -- it shares no code with the kernels.

Link poses come from the CPU oracle's rigid-body states with the root at the
origin (tests/oracle_lib.rigid_body_states, as tests/id_ref.Kinematics takes
them); the root position is added in float64.  Everything after the oracle is
float64.

Besides heights and normals every sample gets its margin, in cells, to the
nearest discontinuity of the output asked for, so that a test can leave out
the few samples at which an fp32 coordinate may fall on the other side:
    CELL heights     the cell lines at which the clamped index changes
    normals          the cell lines (the grid border among them), the cell
                     diagonal fu = fv and the H = 0 crossing of the triangle
    SURFACE heights  the grid border only (the surface is continuous elsewhere)
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests.jacobian_ref import quat_R
from tests.oracle_lib import rigid_body_states
from thormang_isaacgym_amd import abi

# heights [rows, cols] float32, vertex (i, j) at (ox + i hs, oy + j hs, vs heights[i][j])
Heightfield = namedtuple("Heightfield", ["heights", "hs", "vs", "ox", "oy"])
Scan = namedtuple("Scan", ["heights", "normals", "margin", "margin_normals", "xy", "frame_points", "raw"])

MARGIN_CELLS = 1e-3       # samples nearer than this to a discontinuity are left out of a parity check
EXCLUDED_CAP = 0.02       # and they may be at most this share of a case


def reference_pattern():
    """The 14 x 10 pattern of the reference's init_height_points (anymal_terrain.py:503-504), [140, 2] float32 in
    its order: torch.meshgrid(x, y) with ij indexing, flattened."""
    y = 0.1 * np.array([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], np.float32)
    x = 0.1 * np.array([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8], np.float32)
    gx, gy = np.meshgrid(x, y, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.float32)


def frame_poses(m, root, dof, frames, desc=None):
    """(p [N, F, 3], R [N, F, 3, 3]) float64: the frame points p_f = o_l + R_l offset_f in the world and their
    links' rotations.  ``frames``: (link index, offset) pairs."""
    desc = desc or abi.ModelDesc(m)
    root = np.asarray(root, np.float32)
    r0 = root.copy()
    r0[:, :3] = 0.0
    rb = rigid_body_states(desc, r0, np.asarray(dof, np.float32)).astype(np.float64)
    n = root.shape[0]
    p, R = np.zeros((n, len(frames), 3)), np.zeros((n, len(frames), 3, 3))
    for e in range(n):
        for f, (l, off) in enumerate(frames):
            R[e, f] = quat_R(rb[e, l, 3:7] / np.linalg.norm(rb[e, l, 3:7]))
            p[e, f] = root[e, :3].astype(np.float64) + rb[e, l, :3] + R[e, f] @ np.asarray(off, np.float64)
    return p, R


def yaw_matrix(R):
    """The 2 x 2 block of Rz(psi), psi the heading of R: (cos, sin) = (R00 + R11, R10 - R01) normalised, the
    identity when both vanish (the reference's quat_apply_yaw)."""
    c, s = R[0, 0] + R[1, 1], R[1, 0] - R[0, 1]
    nrm = np.hypot(c, s)
    if nrm == 0.0:
        return np.eye(2)
    c, s = c / nrm, s / nrm
    return np.array([[c, -s], [s, c]])


def sample_points(p, R, points, align):
    """World (x, y) of every sample, [N, F, P, 2] float64."""
    pts = np.asarray(points, np.float64)
    n, F = p.shape[:2]
    xy = np.zeros((n, F, pts.shape[0], 2))
    for e in range(n):
        for f in range(F):
            A = {"world": np.eye(2), "link": R[e, f, :2, :2], "yaw": yaw_matrix(R[e, f])}[align]
            xy[e, f] = p[e, f, :2] + pts @ A.T
    return xy


def _cell(hf, x, y):
    H = np.asarray(hf.heights, np.float64)
    rows, cols = H.shape
    u, v = (x - float(hf.ox)) / float(hf.hs), (y - float(hf.oy)) / float(hf.hs)
    return H, rows, cols, u, v


def surface_at(hf, x, y):
    """ground_at at the world points (x, y) (arrays of one shape): (h, n [..., 3], margin of the heights, margin of
    the normals)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    h, nrm = np.zeros(x.shape), np.zeros(x.shape + (3,))
    nrm[..., 2] = 1.0
    inf = np.full(x.shape, np.inf)
    if hf is None:
        return h, nrm, inf, inf.copy()
    H, rows, cols, u, v = _cell(hf, x, y)
    on = (u >= 0) & (v >= 0) & (u <= rows - 1) & (v <= cols - 1)
    du = np.maximum(np.maximum(-u, u - (rows - 1)), 0.0)
    dv = np.maximum(np.maximum(-v, v - (cols - 1)), 0.0)
    inside = np.minimum(np.minimum(u, rows - 1 - u), np.minimum(v, cols - 1 - v))
    m_border = np.where(on, inside, np.hypot(du, dv))
    i = np.clip(np.floor(np.where(on, u, 0.0)), 0, rows - 2).astype(int)
    j = np.clip(np.floor(np.where(on, v, 0.0)), 0, cols - 2).astype(int)
    fu, fv = u - i, v - j
    vs = float(hf.vs)
    h00, h01, h10, h11 = vs * H[i, j], vs * H[i, j + 1], vs * H[i + 1, j], vs * H[i + 1, j + 1]
    low = fu >= fv
    gx, gy = np.where(low, h10 - h00, h11 - h01), np.where(low, h11 - h10, h01 - h00)
    Hs = h00 + fu * gx + fv * gy
    terrain = on & (Hs > 0)
    h = np.where(terrain, Hs, 0.0)
    sx, sy = gx / float(hf.hs), gy / float(hf.hs)
    inv = 1.0 / np.sqrt(sx * sx + sy * sy + 1.0)
    nrm[..., 0] = np.where(terrain, -sx * inv, 0.0)
    nrm[..., 1] = np.where(terrain, -sy * inv, 0.0)
    nrm[..., 2] = np.where(terrain, inv, 1.0)
    m_lines = np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))
    m_diag = np.abs(fu - fv) / np.sqrt(2.0)
    g = np.hypot(gx, gy)
    with np.errstate(divide="ignore", invalid="ignore"):
        m_zero = np.where(g > 0, np.abs(Hs) / np.where(g > 0, g, 1.0), np.inf)
    m_n = np.where(on, np.minimum(np.minimum(m_lines, m_diag), m_zero), m_border)
    return h, nrm, m_border, m_n


def cell_at(hf, x, y):
    """The reference's rule (anymal_terrain.py:524-536): (h, margin)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if hf is None:
        return np.zeros(x.shape), np.full(x.shape, np.inf)
    H, rows, cols, u, v = _cell(hf, x, y)
    i = np.clip(np.trunc(u), 0, rows - 2).astype(int)
    j = np.clip(np.trunc(v), 0, cols - 2).astype(int)
    h = float(hf.vs) * np.minimum(H[i, j], H[i + 1, j + 1])

    def lines(w, cnt):   # the index changes at w = 1 .. cnt - 2
        if cnt < 3:
            return np.full(w.shape, np.inf)
        return np.abs(w - np.clip(np.rint(w), 1, cnt - 2))
    return h, np.minimum(lines(u, rows), lines(v, cols))


def height_scan_ref(m, root, dof, frames, points, hf=None, surface="surface", align="yaw", relative=None, desc=None):
    """Scan(heights [N, F, P], normals [N, F, P, 3] or None, margin [N, F, P] of the heights, margin_normals, xy
    [N, F, P, 2], frame_points [N, F, 3], raw [N, F, P]: h before the relative map), float64.  ``relative``: None
    or dict(bias, lo, hi, scale)."""
    p, R = frame_poses(m, root, dof, frames, desc)
    xy = sample_points(p, R, points, align)
    if surface == "surface":
        h, nrm, mh, mn = surface_at(hf, xy[..., 0], xy[..., 1])
    else:
        h, mh = cell_at(hf, xy[..., 0], xy[..., 1])
        nrm, mn = None, None
    raw = h
    if relative is not None:
        h = np.clip(p[:, :, None, 2] - float(relative["bias"]) - h, float(relative["lo"]), float(relative["hi"])) \
            * float(relative["scale"])
    return Scan(h, nrm, mh, mn, xy, p, raw)


def smooth_heightfield(rows, cols, rs, hs=0.25, vs=0.005, ox=-7.0, oy=-4.5, amp=0.3, shift=0.08):
    """A smooth random terrain: a few sinusoids of wavelengths of 3 .. 8 m, heights within about -amp + shift .. amp +
    shift metres (so that there are negative patches), as raw samples for the vertical scale vs."""
    i, j = np.meshgrid(np.arange(rows) * hs, np.arange(cols) * hs, indexing="ij")
    z = np.zeros((rows, cols))
    for _ in range(4):
        k = rs.uniform(2 * np.pi / 8.0, 2 * np.pi / 3.0)
        th, ph = rs.uniform(0, 2 * np.pi, 2)
        z += np.sin(k * (np.cos(th) * i + np.sin(th) * j) + ph)
    z = amp * z / np.abs(z).max() + shift
    return Heightfield(np.round(z / vs).astype(np.float32), np.float32(hs), np.float32(vs), np.float32(ox),
                       np.float32(oy))
