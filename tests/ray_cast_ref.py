"""float64 reference for the ray cast (tgsim.h tg_ray_cast), a plain numpy
restatement of the header's definitions -- it shares no code with the kernel and
walks no cells: per ray it brute-forces every triangle of the field whose cell
touches the bounding box of the ray's segment (no other triangle has a point
of the segment above it), the four border faces and the plane.  cast_one states
it for one ray; cast_many is the same statement over flat arrays of (ray,
triangle) pairs, which is what the tests run, held to cast_one by
tests/test_ray_cast_reference.py.

Frame poses come from tests/height_scan_ref.frame_poses (the CPU oracle's
rigid-body states with the root at the origin, the root position added in
float64).  Everything after the oracle is float64.

For every triangle the ray's (x, y) is clipped against the triangle's three
edges, which gives the interval of t over it; there f(t) = z(t) - H is linear,
and the first t of the interval with f <= 0 is the triangle's candidate.  The
smallest candidate over all triangles is where the ray enters the terrain solid
{(x, y) on the grid, z <= H}: through a triangle, or -- when it is the very
point at which the ray comes onto the grid -- through the border's vertical
face.  The plane candidate is -o.z / d.z.

Besides dist and normals every ray gets the margins a parity test needs:
    clear     graze clearance, metres: the smallest local minimum of
              z - max(H, 0) (0 for H off the grid) along the ray before the hit
              (before max_range for a miss); the jump at the border counts, so
              the clearance over the border face's top edge is in it
    cos       incidence |d . n| / |d| at the hit (inf on a miss)
    edge      |t_first - max_range| |d|, metres, t_first the first entry into
              the ground looked for a little beyond max_range (inf without one)
    tie_gap   |plane candidate - terrain candidate| |d|, metres (inf with one
              of them missing)
    tie_cells distance of a triangle hit to the nearest cell line or cell
              diagonal, in cells (inf for the other hits and for misses)
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests.height_scan_ref import Heightfield, frame_poses, yaw_matrix  # noqa: F401  (Heightfield re-exported)

Rays = namedtuple("Rays", ["dist", "normals", "clear", "cos", "edge", "tie_gap", "tie_cells", "origin", "direction",
                           "kind", "frame_points"])
# kind: 0 miss, 1 plane, 2 triangle, 3 border face, 4 start inside the ground
MISS, PLANE, TRIANGLE, FACE, INSIDE = 0, 1, 2, 3, 4

COS_MIN = 0.05            # rays that land flatter than this are left out of a parity check
CLEAR = 1e-3              # metres: rays that graze the ground, or end at max_range, nearer than this are left out
MARGIN_CELLS = 1e-3       # normals: hits nearer than this to a cell line or diagonal are left out
EXCLUDED_CAP = 0.02       # and all of them may be at most this share of a case
CLEAR_EXACT = 0.5         # cast_many: a graze clearance under this is exact; one over it is reported as at least this
BEYOND = 0.01             # how far past max_range (in t |d|, metres) the first entry is still looked for


def lidar_pattern(azimuths, elevations):
    """[E * A, 6] float32: unit directions (cos e cos a, cos e sin a, sin e), starts zero, elevation-major."""
    a, e = np.asarray(azimuths, np.float64).ravel(), np.asarray(elevations, np.float64).ravel()
    ee, aa = np.meshgrid(e, a, indexing="ij")
    d = np.stack([np.cos(ee) * np.cos(aa), np.cos(ee) * np.sin(aa), np.sin(ee)], -1).reshape(-1, 3)
    return np.concatenate([np.zeros_like(d), d], 1).astype(np.float32)


def pinhole_pattern(width, height, hfov):
    """[H * W, 6] float32: x forward, y left, z up, row-major from the top-left pixel, d.x = 1."""
    W, H, T = int(width), int(height), np.tan(0.5 * float(hfov))
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([np.ones_like(cc), T * (1 - 2 * (cc + 0.5) / W), T * (H / W) * (1 - 2 * (rr + 0.5) / H)], -1)
    d = d.reshape(-1, 3)
    return np.concatenate([np.zeros_like(d), d], 1).astype(np.float32)


def align_matrix(R, align):
    if align == "link":
        return np.asarray(R, np.float64)
    A = np.eye(3)
    if align == "yaw":
        A[:2, :2] = yaw_matrix(R)
    elif align != "world":
        raise ValueError(align)
    return A


def _scaled(hf):
    """The vertex heights in metres, float64 (a field that already holds them -- vs = 1, float64 -- is not copied)."""
    H = np.asarray(hf.heights)
    return H if H.dtype == np.float64 and float(hf.vs) == 1.0 else H.astype(np.float64) * float(hf.vs)


def _height(hf, u, v):
    """The triangle height H and its gradient per cell (gx, gy) at the cell coordinates (u, v) on the closed grid."""
    Hs = _scaled(hf)
    rows, cols = Hs.shape
    i = int(np.clip(np.floor(u), 0, rows - 2))
    j = int(np.clip(np.floor(v), 0, cols - 2))
    fu, fv = u - i, v - j
    h00, h01, h10, h11 = Hs[i, j], Hs[i, j + 1], Hs[i + 1, j], Hs[i + 1, j + 1]
    gx, gy = (h10 - h00, h11 - h10) if fu >= fv else (h11 - h01, h01 - h00)
    return h00 + fu * gx + fv * gy, gx, gy


def _unit_normal(gx, gy, hs):
    sx, sy = gx / hs, gy / hs
    inv = 1.0 / np.sqrt(sx * sx + sy * sy + 1.0)
    return np.array([-sx * inv, -sy * inv, inv])


def _clip(lo, hi, c0, c1):
    """Intersect [lo, hi] (arrays) with {t: c0 + c1 t >= 0}."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = -c0 / c1
    lo = np.where(c1 > 0, np.maximum(lo, r), lo)
    hi = np.where(c1 < 0, np.minimum(hi, r), hi)
    dead = (c1 == 0) & (c0 < 0)
    return np.where(dead, np.inf, lo), np.where(dead, -np.inf, hi)


def _terrain_pieces(hf, o, d, tlim):
    """Every triangle the segment x(t), t in [0, tlim], passes over: (ta, tb, c0, c1, gx, gy) arrays, f(t) = c0 +
    c1 t on [ta, tb], gradient per cell."""
    Hs = _scaled(hf)
    rows, cols = Hs.shape
    hs = float(hf.hs)
    U0, V0 = (o[0] - float(hf.ox)) / hs, (o[1] - float(hf.oy)) / hs
    dU, dV = d[0] / hs, d[1] / hs
    U1, V1 = U0 + tlim * dU, V0 + tlim * dV
    i0 = int(np.clip(np.floor(min(U0, U1)) - 1, 0, rows - 2))
    i1 = int(np.clip(np.floor(max(U0, U1)) + 1, 0, rows - 2))
    j0 = int(np.clip(np.floor(min(V0, V1)) - 1, 0, cols - 2))
    j1 = int(np.clip(np.floor(max(V0, V1)) + 1, 0, cols - 2))
    if min(U0, U1) > rows - 1 or max(U0, U1) < 0 or min(V0, V1) > cols - 1 or max(V0, V1) < 0:
        return None
    ii, jj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    h00, h01, h10, h11 = Hs[ii, jj], Hs[ii, jj + 1], Hs[ii + 1, jj], Hs[ii + 1, jj + 1]
    a0, b0 = U0 - ii, V0 - jj                     # fu = a0 + t dU, fv = b0 + t dV
    out = []
    for lower in (True, False):
        lo, hi = np.zeros(ii.shape), np.full(ii.shape, float(tlim))
        if lower:      # fv >= 0, fu <= 1, fu - fv >= 0
            gx, gy = h10 - h00, h11 - h10
            lo, hi = _clip(lo, hi, b0, dV)
            lo, hi = _clip(lo, hi, 1.0 - a0, -dU)
            lo, hi = _clip(lo, hi, a0 - b0, dU - dV)
        else:          # fu >= 0, fv <= 1, fv - fu >= 0
            gx, gy = h11 - h01, h01 - h00
            lo, hi = _clip(lo, hi, a0, dU)
            lo, hi = _clip(lo, hi, 1.0 - b0, -dV)
            lo, hi = _clip(lo, hi, b0 - a0, dV - dU)
        ok = lo <= hi
        c0 = o[2] - (h00 + a0 * gx + b0 * gy)
        c1 = d[2] - (dU * gx + dV * gy)
        out.append(np.stack([lo, hi, c0, c1, gx, gy], 1)[ok])
    pcs = np.concatenate(out, 0)
    return pcs if len(pcs) else None


def _grid_span(hf, o, d, tlim):
    """(t_in, t_out, face normal of the entry or None): the part of [0, tlim] over the closed grid rectangle."""
    rows, cols = np.asarray(hf.heights).shape
    hs = float(hf.hs)
    lo, hi, face = 0.0, float(tlim), None
    for axis, (p0, dp, top) in enumerate((((o[0] - float(hf.ox)) / hs, d[0] / hs, rows - 1.0),
                                          ((o[1] - float(hf.oy)) / hs, d[1] / hs, cols - 1.0))):
        if dp == 0.0:
            if p0 < 0 or p0 > top:
                return None
            continue
        ta, tb = sorted(((0.0 - p0) / dp, (top - p0) / dp))
        if ta > lo:                                  # strictly: the x face wins at a corner
            lo = ta
            face = np.zeros(3)
            face[axis] = -np.sign(dp)
        hi = min(hi, tb)
    return (lo, hi, face) if lo <= hi else None


def cast_one(hf, o, d, max_range):
    """One ray against the ground: dict(dist, normal, kind, clear, cos, edge, tie_gap, tie_cells)."""
    miss = dict(dist=float(max_range), normal=np.zeros(3), kind=MISS, clear=np.inf, cos=np.inf, edge=np.inf,
                tie_gap=np.inf, tie_cells=np.inf)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    if not (np.isfinite(o).all() and np.isfinite(d).all()) or not d.any():
        return miss
    nd = float(np.linalg.norm(d))
    tlim = float(max_range) + BEYOND / nd
    hs = float(hf.hs) if hf is not None else 1.0
    # the start
    H0, n0 = 0.0, np.array([0.0, 0.0, 1.0])
    if hf is not None:
        rows, cols = np.asarray(hf.heights).shape
        u, v = (o[0] - float(hf.ox)) / hs, (o[1] - float(hf.oy)) / hs
        if 0 <= u <= rows - 1 and 0 <= v <= cols - 1:
            H, gx, gy = _height(hf, u, v)
            if H > 0:
                H0, n0 = H, _unit_normal(gx, gy, hs)
    if o[2] <= H0:
        return dict(miss, dist=0.0, normal=n0, kind=INSIDE, cos=abs(float(d @ n0)) / nd, edge=float(max_range) * nd)
    # candidates
    t_plane = -o[2] / d[2] if d[2] < 0 else np.inf
    t_mesh, n_mesh, kind_mesh, cells = np.inf, None, MISS, np.inf
    pcs = span = None
    if hf is not None:
        tl = min(tlim, float(t_plane))               # nothing of the terrain solid is entered after the plane
        span = _grid_span(hf, o, d, tl)
        pcs = _terrain_pieces(hf, o, d, tl) if span is not None else None
    if pcs is not None:
        ta, tb, c0, c1 = pcs[:, 0], pcs[:, 1], pcs[:, 2], pcs[:, 3]
        fa, fb = c0 + ta * c1, c0 + tb * c1
        with np.errstate(divide="ignore", invalid="ignore"):
            root = np.clip(-c0 / c1, ta, tb)
        cand = np.where(fa <= 0, ta, np.where(fb <= 0, root, np.inf))
        k = int(np.argmin(cand))
        if np.isfinite(cand[k]):
            t_mesh = float(cand[k])
            n_mesh, kind_mesh = _unit_normal(pcs[k, 4], pcs[k, 5], hs), TRIANGLE
            t_in, _t_out, face = span
            # in the solid at the very point it comes onto the grid: the border's face
            if face is not None and t_mesh <= t_in + 1e-12 * (1.0 + abs(t_in)):
                n_mesh, kind_mesh = face, FACE
            else:
                u = (o[0] + t_mesh * d[0] - float(hf.ox)) / hs
                v = (o[1] + t_mesh * d[1] - float(hf.oy)) / hs
                fu, fv = u - np.floor(u), v - np.floor(v)
                cells = min(abs(u - np.rint(u)), abs(v - np.rint(v)), abs(fu - fv) / np.sqrt(2.0))
    t_first = min(t_plane, t_mesh)
    res = dict(miss)
    res["tie_gap"] = abs(t_plane - t_mesh) * nd if np.isfinite(t_plane) and np.isfinite(t_mesh) else np.inf
    res["edge"] = abs(t_first - float(max_range)) * nd if np.isfinite(t_first) and t_first <= tlim else np.inf
    t_end = float(max_range)
    if t_first < max_range:
        t_end = t_first
        if t_mesh < t_plane:
            res.update(dist=t_mesh, normal=n_mesh, kind=kind_mesh, tie_cells=cells if kind_mesh == TRIANGLE else np.inf)
        else:
            res.update(dist=t_plane, normal=np.array([0.0, 0.0, 1.0]), kind=PLANE)
        res["cos"] = abs(float(d @ res["normal"])) / nd
    res["clear"] = _clearance(o, d, span, pcs, t_end, res["kind"] != MISS)
    return res


def _clearance(o, d, span, pcs, t_end, hit):
    """The smallest local minimum of g(t) = z - max(H, 0) on [0, t_end] before the final descent into the hit."""
    pieces = []                                      # (ta, tb, g(ta), g(tb)) of every linear piece, in ray order

    def plain(ta, tb):
        ta, tb = max(ta, 0.0), min(tb, t_end)
        if ta <= tb:
            pieces.append((ta, tb, o[2] + ta * d[2], o[2] + tb * d[2]))
    if span is None or pcs is None:
        plain(0.0, t_end)
    else:
        t_in, t_out, _face = span
        if t_in > 0:
            plain(0.0, t_in)
        if t_out < t_end:
            plain(t_out, t_end)
        ta, tb = np.maximum(pcs[:, 0], 0.0), np.minimum(pcs[:, 1], t_end)
        ok = ta <= tb
        ta, tb, c0, c1 = ta[ok], tb[ok], pcs[ok, 2], pcs[ok, 3]
        za, zb = o[2] + ta * d[2], o[2] + tb * d[2]
        # z - max(H, 0) = min(f, z): both linear, so the piece may break once where H crosses 0 (f = z)
        ga, gb = np.minimum(c0 + ta * c1, za), np.minimum(c0 + tb * c1, zb)
        for k in range(len(ta)):
            pieces.append((ta[k], tb[k], ga[k], gb[k]))
    if not pieces:
        return np.inf
    pieces.sort(key=lambda p: (0.5 * (p[0] + p[1]), p[0]))
    g = np.array([x for p in pieces for x in (p[2], p[3])])
    if not hit:
        return float(g.min())
    m = len(g) - 1
    while m > 0 and g[m - 1] >= g[m]:
        m -= 1
    return float(g[:m].min()) if m > 0 else np.inf


def _first_per_group(gid, key, n):
    """Index, into the arrays, of each group's element with the smallest key (-1 for an empty group): groups 0..n-1."""
    order = np.lexsort((key, gid))
    start = np.searchsorted(gid[order], np.arange(n), side="left")
    stop = np.searchsorted(gid[order], np.arange(n), side="right")
    return np.where(stop > start, order[np.minimum(start, len(order) - 1)] if len(order) else -1, -1)


def _group_min(gid, val, n):
    out = np.full(n, np.inf)
    np.minimum.at(out, gid, val)
    return out


def cast_many(hf, O, D, max_range, budget=1_500_000):
    """cast_one for the rays (O [M, 3], D [M, 3]) at once -- the same statement, the same brute force over every
    triangle under each ray's bounding box, with the (ray, triangle) pairs of a batch of rays laid out in flat arrays
    instead of a Python loop per ray.  One cut keeps the arrays small: where a ray is more than CLEAR_EXACT above the
    highest vertex it can neither hit the terrain nor graze it, so only the rest of the ray is laid against the
    triangles; a graze clearance under CLEAR_EXACT is cast_one's, a larger one is reported as at least CLEAR_EXACT
    (the tests compare it with CLEAR = 1 mm only).  Returns a dict of arrays (dist, normal [M, 3], kind, clear, cos, edge, tie_gap,
    tie_cells).  tests/test_ray_cast_reference.py holds it to cast_one."""
    O, D = np.asarray(O, np.float64).reshape(-1, 3), np.asarray(D, np.float64).reshape(-1, 3)
    M = O.shape[0]
    res = dict(dist=np.full(M, float(max_range)), normal=np.zeros((M, 3)), kind=np.zeros(M, int),
               clear=np.full(M, np.inf), cos=np.full(M, np.inf), edge=np.full(M, np.inf),
               tie_gap=np.full(M, np.inf), tie_cells=np.full(M, np.inf))
    if hf is not None:
        hf = Heightfield(_scaled(hf), float(hf.hs), 1.0, float(hf.ox), float(hf.oy))
        # batches of rays whose bounding boxes hold at most ``budget`` cells together
        rows, cols = hf.heights.shape
        span = np.nan_to_num(np.abs(D[:, :2]) * (float(max_range) + 1.0) / hf.hs, nan=0.0, posinf=0.0) + 3.0
        cells = np.minimum(span[:, 0], rows) * np.minimum(span[:, 1], cols)
        edges, acc, a = [0], 0.0, 0
        for k in range(M):
            acc += cells[k]
            if acc > budget and k > a:
                edges.append(k)
                a, acc = k, cells[k]
        edges.append(M)
    else:
        edges = [0, M]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a, b in zip(edges[:-1], edges[1:]):
            part = _cast_batch(hf, O[a:b], D[a:b], float(max_range))
            for key in res:
                res[key][a:b] = part[key]
    return res


def _cast_batch(hf, O, D, max_range):
    M = O.shape[0]
    ez = np.array([0.0, 0.0, 1.0])
    dist, normal, kind = np.full(M, max_range), np.zeros((M, 3)), np.zeros(M, int)
    clear, cos, edge = np.full(M, np.inf), np.full(M, np.inf), np.full(M, np.inf)
    tie_gap, tie_cells = np.full(M, np.inf), np.full(M, np.inf)
    valid = np.isfinite(O).all(1) & np.isfinite(D).all(1) & D.any(1)
    Ov, Dv = np.where(valid[:, None], O, 1.0), np.where(valid[:, None], D, ez)     # (placeholders where invalid)
    nd = np.linalg.norm(Dv, axis=1)
    tlim = max_range + BEYOND / nd
    oz, dz = Ov[:, 2], Dv[:, 2]
    H0, n0 = np.zeros(M), np.tile(ez, (M, 1))
    if hf is not None:
        Hs, hs = hf.heights, float(hf.hs)
        rows, cols = Hs.shape
        U0, V0 = (Ov[:, 0] - float(hf.ox)) / hs, (Ov[:, 1] - float(hf.oy)) / hs
        dU, dV = Dv[:, 0] / hs, Dv[:, 1] / hs
        on = (U0 >= 0) & (U0 <= rows - 1) & (V0 >= 0) & (V0 <= cols - 1)
        i = np.clip(np.floor(np.where(on, U0, 0.0)), 0, rows - 2).astype(int)
        j = np.clip(np.floor(np.where(on, V0, 0.0)), 0, cols - 2).astype(int)
        fu, fv = U0 - i, V0 - j
        h00, h01, h10, h11 = Hs[i, j], Hs[i, j + 1], Hs[i + 1, j], Hs[i + 1, j + 1]
        low = fu >= fv
        gx, gy = np.where(low, h10 - h00, h11 - h01), np.where(low, h11 - h10, h01 - h00)
        H = h00 + fu * gx + fv * gy
        up = on & (H > 0)
        H0 = np.where(up, H, 0.0)
        sx, sy = gx / hs, gy / hs
        inv = 1.0 / np.sqrt(sx * sx + sy * sy + 1.0)
        n0 = np.where(up[:, None], np.stack([-sx * inv, -sy * inv, inv], 1), n0)
    inside = valid & (oz <= H0)
    live = valid & ~inside
    t_plane = np.where(dz < 0, -oz / np.where(dz < 0, dz, -1.0), np.inf)
    t_mesh, n_mesh, face_hit, cells = np.full(M, np.inf), np.zeros((M, 3)), np.zeros(M, bool), np.full(M, np.inf)
    pieces = None                    # rid, ta, tb, c0, c1 of every triangle piece
    t_in, t_out, has_span = np.zeros(M), np.zeros(M), np.zeros(M, bool)
    tA, tB = np.zeros(M), np.full(M, np.inf)
    if hf is not None:
        tl = np.minimum(tlim, t_plane)               # nothing of the terrain solid is entered after the plane
        # the part of [0, tl] over the closed grid rectangle, and the face it is entered through
        t_in, t_out, face = np.zeros(M), tl.copy(), np.zeros((M, 3))
        has_span = live.copy()
        for axis, (p0, dp, top) in enumerate(((U0, dU, rows - 1.0), (V0, dV, cols - 1.0))):
            safe = np.where(dp != 0, dp, 1.0)
            ta, tb = (0.0 - p0) / safe, (top - p0) / safe
            lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
            moving = dp != 0
            has_span &= moving | ((p0 >= 0) & (p0 <= top))
            later = moving & (lo > t_in)             # strictly: the x face wins at a corner
            t_in = np.where(later, lo, t_in)
            face[later] = 0.0
            face[later, axis] = -np.sign(dp[later])
            t_out = np.where(moving, np.minimum(t_out, hi), t_out)
        has_span &= t_in <= t_out
        has_face = face.any(1)
        # no triangle has a point at or under the ray where z(t) > max H, and there z - max(H, 0) > CLEAR_EXACT too:
        # only [tA, tB], the part of [0, tl] with z(t) <= max(H, 0) + CLEAR_EXACT, can hold a hit or a clearance
        # under CLEAR_EXACT
        zcut = max(float(Hs.max()), 0.0) + CLEAR_EXACT
        tz = (zcut - oz) / np.where(dz != 0, dz, 1.0)
        tA = np.where(dz < 0, np.maximum(tz, 0.0), 0.0)
        tB = np.where(dz > 0, np.minimum(tz, tl), np.where((dz == 0) & (oz > zcut), -1.0, tl))
        # every cell the bounding box of the segment [tA, tB] touches
        UA, VA, U1, V1 = U0 + tA * dU, V0 + tA * dV, U0 + tB * dU, V0 + tB * dV
        umin, umax, vmin, vmax = np.minimum(UA, U1), np.maximum(UA, U1), np.minimum(VA, V1), np.maximum(VA, V1)
        boxed = has_span & (tA <= tB) & ~((umin > rows - 1) | (umax < 0) | (vmin > cols - 1) | (vmax < 0))
        fl = lambda x, n: np.clip(np.floor(np.where(boxed, x, 0.0)), 0, n).astype(int)      # noqa: E731
        i0, i1 = fl(umin - 1, rows - 2), fl(umax + 1, rows - 2)
        j0, j1 = fl(vmin - 1, cols - 2), fl(vmax + 1, cols - 2)
        ni, nj = np.where(boxed, i1 - i0 + 1, 0), np.where(boxed, j1 - j0 + 1, 0)
        cnt = ni * nj
        rid = np.repeat(np.arange(M), cnt)
        q = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ii, jj = i0[rid] + q // np.maximum(nj[rid], 1), j0[rid] + q % np.maximum(nj[rid], 1)
        h00, h01, h10, h11 = Hs[ii, jj], Hs[ii, jj + 1], Hs[ii + 1, jj], Hs[ii + 1, jj + 1]
        a0, b0 = U0[rid] - ii, V0[rid] - jj          # fu = a0 + t dU, fv = b0 + t dV
        du, dv = dU[rid], dV[rid]
        parts = []
        for lower in (True, False):
            lo, hi = tA[rid].copy(), tB[rid].copy()
            if lower:      # fv >= 0, fu <= 1, fu - fv >= 0
                gx, gy = h10 - h00, h11 - h10
                lo, hi = _clip(lo, hi, b0, dv)
                lo, hi = _clip(lo, hi, 1.0 - a0, -du)
                lo, hi = _clip(lo, hi, a0 - b0, du - dv)
            else:          # fu >= 0, fv <= 1, fv - fu >= 0
                gx, gy = h11 - h01, h01 - h00
                lo, hi = _clip(lo, hi, a0, du)
                lo, hi = _clip(lo, hi, 1.0 - b0, -dv)
                lo, hi = _clip(lo, hi, b0 - a0, dv - du)
            ok = lo <= hi
            c0 = oz[rid] - (h00 + a0 * gx + b0 * gy)
            c1 = dz[rid] - (du * gx + dv * gy)
            parts.append(np.stack([rid[ok], lo[ok], hi[ok], c0[ok], c1[ok], gx[ok], gy[ok]], 1))
        P = np.concatenate(parts, 0)
        if len(P):
            prid = P[:, 0].astype(int)
            ta, tb, c0, c1 = P[:, 1], P[:, 2], P[:, 3], P[:, 4]
            fa, fb = c0 + ta * c1, c0 + tb * c1
            root = np.clip(-c0 / c1, ta, tb)
            cand = np.where(fa <= 0, ta, np.where(fb <= 0, root, np.inf))
            k = _first_per_group(prid, cand, M)
            got = (k >= 0) & np.isfinite(cand[np.maximum(k, 0)])
            kk = np.maximum(k, 0)
            t_mesh = np.where(got, cand[kk], np.inf)
            sx, sy = P[kk, 5] / hs, P[kk, 6] / hs
            inv = 1.0 / np.sqrt(sx * sx + sy * sy + 1.0)
            n_mesh = np.stack([-sx * inv, -sy * inv, inv], 1)
            # in the solid at the very point it comes onto the grid: the border's face
            face_hit = got & has_face & (t_mesh <= t_in + 1e-12 * (1.0 + np.abs(t_in)))
            n_mesh = np.where(face_hit[:, None], face, n_mesh)
            tm = np.where(got, t_mesh, 0.0)
            u, v = U0 + tm * dU, V0 + tm * dV
            fu, fv = u - np.floor(u), v - np.floor(v)
            cells = np.where(got & ~face_hit, np.minimum(np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v))),
                                                         np.abs(fu - fv) / np.sqrt(2.0)), np.inf)
            pieces = (prid, ta, tb, c0, c1)
    t_first = np.minimum(t_plane, t_mesh)
    both = np.isfinite(t_plane) & np.isfinite(t_mesh)
    tie_gap = np.where(live & both, np.abs(np.where(both, t_plane - t_mesh, 0.0)) * nd, np.inf)
    seen = live & np.isfinite(t_first) & (t_first <= tlim)
    edge = np.where(seen, np.abs(np.where(seen, t_first, 0.0) - max_range) * nd, np.inf)
    hit = live & (t_first < max_range)
    mesh = hit & (t_mesh < t_plane)
    plane = hit & ~mesh
    dist = np.where(hit, t_first, max_range)
    normal = np.where(mesh[:, None], n_mesh, np.where(plane[:, None], ez, 0.0))
    kind = np.where(mesh, np.where(face_hit, FACE, TRIANGLE), np.where(plane, PLANE, MISS))
    tie_cells = np.where(mesh & ~face_hit, cells, np.inf)
    cos = np.where(hit, np.abs((Dv * normal).sum(1)) / nd, np.inf)
    # a start inside the ground
    dist = np.where(inside, 0.0, dist)
    normal = np.where(inside[:, None], n0, normal)
    kind = np.where(inside, INSIDE, kind)
    cos = np.where(inside, np.abs((Dv * n0).sum(1)) / nd, cos)
    edge = np.where(inside, max_range * nd, edge)
    tie_gap = np.where(inside, np.inf, tie_gap)
    # graze clearance: every linear piece of g(t) = z - max(H, 0) on [0, t_end], in ray order
    t_end = np.where(hit, t_first, max_range)
    has_pcs = np.zeros(M, bool)
    if pieces is not None:
        has_pcs[np.unique(pieces[0])] = True
    G = []                                           # (rid, ta, tb, ga, gb)

    def plain(sel, ta, tb):
        ta, tb = np.maximum(ta, tA), np.minimum(tb, np.minimum(t_end, tB))
        ok = sel & (ta <= tb)
        r = np.nonzero(ok)[0]
        G.append(np.stack([r, ta[r], tb[r], oz[r] + ta[r] * dz[r], oz[r] + tb[r] * dz[r]], 1))
    on_terrain = live & has_span & has_pcs
    plain(live & ~on_terrain, np.zeros(M), t_end)
    plain(on_terrain & (t_in > 0), np.zeros(M), t_in)
    plain(on_terrain & (t_out < t_end), t_out, t_end)
    if pieces is not None:
        prid, ta, tb, c0, c1 = pieces
        ta, tb = np.maximum(ta, 0.0), np.minimum(tb, t_end[prid])
        ok = (ta <= tb) & on_terrain[prid]
        prid, ta, tb, c0, c1 = prid[ok], ta[ok], tb[ok], c0[ok], c1[ok]
        za, zb = oz[prid] + ta * dz[prid], oz[prid] + tb * dz[prid]
        # z - max(H, 0) = min(f, z): both linear, so the piece may break once where H crosses 0 (f = z)
        G.append(np.stack([prid, ta, tb, np.minimum(c0 + ta * c1, za), np.minimum(c0 + tb * c1, zb)], 1))
    G = np.concatenate(G, 0)
    if len(G):
        order = np.lexsort((G[:, 1], 0.5 * (G[:, 1] + G[:, 2]), G[:, 0]))
        G = G[order]
        gr = np.repeat(G[:, 0].astype(int), 2)
        g = G[:, 3:5].reshape(-1)
        idx = np.arange(len(g))
        rise = np.zeros(len(g), bool)
        rise[1:] = (g[1:] > g[:-1]) & (gr[1:] == gr[:-1])
        last = np.full(M, -1)
        np.maximum.at(last, gr, np.where(rise, idx, -1))          # a hit's final descent starts at its last rise
        before = np.where(hit[gr], idx < last[gr], True)
        clear = np.where(live, _group_min(gr[before], g[before], M), np.inf)
    return dict(dist=dist, normal=normal, kind=kind, clear=clear, cos=cos, edge=edge, tie_gap=tie_gap,
                tie_cells=tie_cells)


def ray_cast_ref(m, root, dof, frames, rays, hf=None, align="link", max_range=20.0, desc=None):
    """Rays(dist [N, F, R], normals [N, F, R, 3], clear, cos, edge, tie_gap, tie_cells, origin [N, F, R, 3], direction,
    kind [N, F, R] int, frame_points [N, F, 3]), float64."""
    p, Rm = frame_poses(m, root, dof, frames, desc)
    return cast_from_poses(p, Rm, rays, hf, align, max_range)


def cast_from_poses(p, Rm, rays, hf=None, align="link", max_range=20.0):
    """The pattern cast from the frame poses (p [N, F, 3], Rm [N, F, 3, 3]): every ray through cast_many."""
    rays = np.asarray(rays, np.float64)
    n, F = p.shape[:2]
    R = rays.shape[0]
    shape = (n, F, R)
    A = np.array([[align_matrix(Rm[e, f], align) for f in range(F)] for e in range(n)])       # [N, F, 3, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        org = p[:, :, None, :] + np.einsum("efij,kj->efki", A, rays[:, :3])
        dirs = np.einsum("efij,kj->efki", A, rays[:, 3:])
    r = cast_many(hf, org.reshape(-1, 3), dirs.reshape(-1, 3), max_range)
    return Rays(r["dist"].reshape(shape), r["normal"].reshape(shape + (3,)), r["clear"].reshape(shape),
                r["cos"].reshape(shape), r["edge"].reshape(shape), r["tie_gap"].reshape(shape),
                r["tie_cells"].reshape(shape), org, dirs, r["kind"].reshape(shape), p)


def keep_dist(r, clear=CLEAR, cos_min=COS_MIN):
    """The rays whose distance a parity check compares."""
    return (r.clear >= clear) & (r.cos >= cos_min) & (r.edge >= clear)


def keep_normals(r, clear=CLEAR, cos_min=COS_MIN, cells=MARGIN_CELLS):
    """The rays whose normal a parity check compares."""
    return keep_dist(r, clear, cos_min) & (r.tie_gap >= clear) & (r.tie_cells >= cells)
