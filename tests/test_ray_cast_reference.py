"""The float64 reference of the ray cast (tests/ray_cast_ref.py) pinned without
a GPU: hand-known answers on a plateau whose every coordinate is exact, the
analytic ray-plane value on a ramp whose triangles are coplanar (rays along a
cell line, along a cell diagonal, parallel to each axis and vertical among
them), the height scan's reference under downward rays, the margins, and the
exclusion cap of tests/test_gpu_ray_cast.py on that file's own inputs.

The plateau (tests/test_gpu_ray_cast.PLATEAU): 5 x 4 samples of raw height 1,
vs = 0.5, hs = 0.25, origin (2, 4) -- the solid x in [2, 3], y in [4, 4.75],
z <= 0.5 on the z = 0 plane.  One free body with the identity rotation stands at
(2.5, 4.25, 0), over the middle of the plateau; the rays' start offsets place
each ray."""
import numpy as np
import pytest

from tests import ray_cast_ref as rr
from tests.height_scan_ref import height_scan_ref, reference_pattern, smooth_heightfield, surface_at
from tests.test_gpu_ray_cast import (ALIGNS, CASES, MAX_RANGE, N, PLATEAU, PLATEAU_RANGE, PLATEAU_ROOT, PLATEAU_TABLE,
                                     RAMP, excluded_shares, patterns, plateau_rays, ramp_analytic, ramp_rays,
                                     reference, scenario, terrain)


def _free_body(roots):
    from tests import physics_models as pm
    m = pm.free_body()
    root = np.zeros((len(roots), 13), np.float32)
    root[:, 6] = 1.0
    root[:, :3] = roots
    return m, root, np.zeros((0, 2), np.float32)


@pytest.mark.parametrize("align", ALIGNS)
def test_plateau_table(align):
    m, root, dof = _free_body([PLATEAU_ROOT])
    r = rr.ray_cast_ref(m, root, dof, [(0, (0.0, 0.0, 0.0))], plateau_rays(), PLATEAU, align, PLATEAU_RANGE)
    for k, (_s, _d, t, n) in enumerate(PLATEAU_TABLE):
        assert r.dist[0, 0, k] == t, (k, r.dist[0, 0, k], t)
        assert np.array_equal(r.normals[0, 0, k], np.asarray(n, np.float64)), (k, r.normals[0, 0, k])
    want = [rr.TRIANGLE, rr.PLANE, rr.FACE, rr.FACE, rr.MISS, rr.MISS, rr.INSIDE, rr.INSIDE, rr.TRIANGLE, rr.TRIANGLE,
            rr.PLANE, rr.MISS, rr.MISS, rr.MISS]          # (the top is terrain, its normal e_z)
    assert r.kind[0, 0].tolist() == want
    # the hit just beyond max_range is seen by its range edge, the miss over the top by its graze clearance
    assert r.edge[0, 0, 11] == pytest.approx(2.0 ** -10) and r.clear[0, 0, 4] == pytest.approx(0.25)
    assert r.clear[0, 0, 10] == pytest.approx(0.25)     # over the top edge at x = 3: z = 0.75 there
    assert np.isinf(r.cos[0, 0, 4]) and r.cos[0, 0, 8] == pytest.approx(np.sqrt(0.5))


def test_plateau_corner_the_x_face_wins():
    m, root, dof = _free_body([PLATEAU_ROOT])
    rays = np.array([[-1.0, -0.75, 0.25, 1.0, 1.0, 0.0]], np.float32)      # from (1.5, 3.5) towards the corner (2, 4)
    r = rr.ray_cast_ref(m, root, dof, [(0, (0.0, 0.0, 0.0))], rays, PLATEAU, "world", PLATEAU_RANGE)
    assert r.dist[0, 0, 0] == 0.5 and np.array_equal(r.normals[0, 0, 0], [-1.0, 0.0, 0.0])


def test_ramp_is_the_analytic_ray_plane_value():
    m, root, dof = _free_body([(2.0, -1.25, 0.0)])
    rays = ramp_rays()
    r = rr.ray_cast_ref(m, root, dof, [(0, (0.0, 0.0, 0.0))], rays, RAMP, "world", 8.0)
    t = ramp_analytic(rays)
    assert np.allclose(r.dist[0, 0], t, rtol=0, atol=1e-12)
    n = np.array([-0.25, -0.125, 1.0]) / np.sqrt(0.25 ** 2 + 0.125 ** 2 + 1.0)
    assert np.allclose(r.normals[0, 0], n, atol=1e-12) and (r.kind[0, 0] == rr.TRIANGLE).all()
    # the rays along cell lines and diagonals have no tie margin, the general ones do
    assert (r.tie_cells[0, 0, :3] < 1e-9).all() and (r.tie_cells[0, 0, -2:] > 1e-3).all()
    # where the ramp is negative the z <= 0 half-space is the ground: a ramp lowered by 0.5 m
    low = RAMP._replace(heights=RAMP.heights - np.float32(64.0))            # -0.5 m: H < 0 for x + y / 2 < 0.75 + ...
    r2 = rr.ray_cast_ref(m, root, dof, [(0, (0.0, 0.0, 0.0))], rays, low, "world", 8.0)
    o = np.asarray([2.0, -1.25, 0.0]) + rays[:, :3].astype(np.float64)
    d = rays[:, 3:].astype(np.float64)
    t_low = ramp_analytic(rays) - 0.5 / (d[:, 2] - d[:, :2] @ np.array([0.25, 0.125]))   # the lowered plane
    t_plane = -o[:, 2] / d[:, 2]
    assert np.allclose(r2.dist[0, 0], np.minimum(t_low, t_plane), atol=1e-12)
    assert (t_plane < t_low).any() and (t_low < t_plane).any()
    assert ((r2.kind[0, 0] == rr.PLANE) == (t_plane < t_low)).all()


@pytest.mark.parametrize("align", ["world", "yaw"])
def test_downward_rays_give_the_height_scans_reference(align):
    from tests import physics_models as pm
    from tests.test_rigid_body_states import random_state
    hf = smooth_heightfield(200, 168, np.random.default_rng(7))
    m = pm.free_body()
    root, dof = random_state(m, 3, np.random.default_rng(4))
    root[:, :2] = [[3.3, 2.2], [20.1, 11.7], [-6.8, 30.2]]
    root[:, 2] = 3.0
    th = np.array([0.3, -1.1, 2.0])
    root[:, 3:7] = np.stack([0 * th, 0 * th, np.sin(th / 2), np.cos(th / 2)], 1)      # level: the frame stays at z = 3
    pts = reference_pattern()
    rays = np.zeros((pts.shape[0], 6), np.float32)
    rays[:, :2], rays[:, 5] = pts, -1.0
    frames = [(0, (0.0, 0.0, 0.0))]
    r = rr.ray_cast_ref(m, root, dof, frames, rays, hf, align, 5.0)
    h = height_scan_ref(m, root, dof, frames, pts, hf, "surface", align)
    assert np.allclose(r.dist, 3.0 - h.heights, rtol=0, atol=1e-12)
    assert (h.heights > 0.05).any() and (h.heights == 0.0).any()
    keep = h.margin_normals >= 1e-6
    assert np.allclose(r.normals[keep], h.normals[keep], atol=1e-12)


def test_the_batched_reference_is_the_per_ray_one():
    """cast_many against cast_one, ray by ray, on the GPU test's terrain: starts inside, axis-parallel, vertical, zero
    and NaN directions, starts on cell lines and rays from outside the border among them.  Everything agrees to
    float64 rounding; a graze clearance agrees when it is under CLEAR_EXACT and both are over it otherwise."""
    rs = np.random.default_rng(1)
    hf = terrain()
    n = 600
    xy = np.stack([rs.uniform(-9, 45, n), rs.uniform(-6, 39, n)], 1)
    o = np.concatenate([xy, (surface_at(hf, xy[:, 0], xy[:, 1])[0] + rs.uniform(0.3, 1.4, n))[:, None]], 1)
    d = rs.normal(0, 1, (n, 3))
    d[:, 2] = 0.05 - 0.3 * np.abs(d[:, 2])
    od = np.concatenate([o, d], 1).astype(np.float32).astype(np.float64)
    od[:40, 2] -= 1.2
    od[40:80, 3] = 0
    od[80:120, 3:5] = 0
    od[120:125, 3:] = 0
    od[125:128, 4] = np.nan
    od[128:200, 0] = np.round((od[128:200, 0] + 7) / 0.25) * 0.25 - 7
    od[200:260, 0] = -7.4
    for field in (hf, None):
        many = rr.cast_many(field, od[:, :3], od[:, 3:], MAX_RANGE, budget=20000)       # (several batches)
        one = [rr.cast_one(field, od[k, :3], od[k, 3:], MAX_RANGE) for k in range(n)]
        assert np.array_equal(many["kind"], [r["kind"] for r in one])
        assert len(set(many["kind"])) == (5 if field is not None else 3)
        for key in ("dist", "cos", "edge", "tie_gap", "tie_cells", "normal"):
            a, b = many[key], np.array([r[key] for r in one])
            assert np.array_equal(np.isinf(a), np.isinf(b)), key
            fin = np.isfinite(a)
            assert np.allclose(a[fin], b[fin], rtol=0, atol=1e-12), key
        a, b = many["clear"], np.array([r["clear"] for r in one])
        small = np.minimum(a, b) < rr.CLEAR_EXACT
        assert np.allclose(a[small], b[small], rtol=0, atol=1e-12) and small.sum() > 50
        assert (a[~small] >= rr.CLEAR_EXACT).all() and (b[~small] >= rr.CLEAR_EXACT).all()


def test_margins():
    m, root, dof = _free_body([PLATEAU_ROOT])
    rays = np.array([
        [-1.5, 0.0, 0.502, 1.0, 0.0, 0.0],          # skims the top 2 mm up: a miss with a graze clearance of 2 mm
        [-1.5, 0.0, 0.25, 1.0, 0.0, -0.125],        # onto the plane before the plateau: t = 2 would be behind the face
        [0.0, 0.0, 1.0, 1.0, 0.0, -1.0],            # lands on the top at 45 degrees, on a cell line and a diagonal
        [0.0625, 0.03125, 1.0, 0.0, 0.0, -1.0],     # lands inside a triangle
    ], np.float32)
    r = rr.ray_cast_ref(m, root, dof, [(0, (0.0, 0.0, 0.0))], rays, PLATEAU, "world", PLATEAU_RANGE)
    assert r.kind[0, 0].tolist() == [rr.MISS, rr.FACE, rr.TRIANGLE, rr.TRIANGLE]
    assert r.clear[0, 0, 0] == pytest.approx(2e-3, rel=1e-3)
    assert r.dist[0, 0, 1] == 1.0 and r.tie_gap[0, 0, 1] == pytest.approx(np.sqrt(1 + 0.125 ** 2))   # plane at t = 2
    assert r.cos[0, 0, 2] == pytest.approx(np.sqrt(0.5)) and r.tie_cells[0, 0, 2] < 1e-12
    assert r.tie_cells[0, 0, 3] == pytest.approx(0.125 / np.sqrt(2.0)) and r.cos[0, 0, 3] == 1.0
    assert r.edge[0, 0, 3] == pytest.approx(PLATEAU_RANGE - 0.5)
    keep_d, keep_n = rr.keep_dist(r)[0, 0], rr.keep_normals(r)[0, 0]
    # (ray 2 lands on the top's very edge at x = 3: a hair further and it would pass on to the plane, so it is a graze)
    assert r.clear[0, 0, 2] == 0.0
    assert keep_d.tolist() == [True, True, False, True] and keep_n.tolist() == [True, True, False, True]


def test_patterns():
    p = patterns()
    lid = p["lidar"]
    assert lid.shape == (96, 6) and not lid[:, :3].any()
    assert np.allclose(np.linalg.norm(lid[:, 3:], axis=1), 1.0, atol=1e-6)
    # elevation-major: the first 16 rays are the -50 degree ring, the azimuth grows within it from 3 degrees
    assert np.allclose(lid[:16, 5], np.sin(np.deg2rad(-50.0)), atol=1e-6)
    assert np.allclose(np.arctan2(lid[0, 4], lid[0, 3]), np.deg2rad(3.0), atol=1e-6)
    assert np.allclose(np.arctan2(lid[1, 4], lid[1, 3]), np.deg2rad(25.5), atol=1e-6)
    pin = rr.pinhole_pattern(4, 2, np.deg2rad(90.0))
    # T = 1; row 0 is the top (z > 0), column 0 the left (y > 0); d.x = 1
    assert np.allclose(pin[:, 3], 1.0) and np.allclose(pin[0, 3:], [1.0, 0.75, 0.25]) and \
        np.allclose(pin[3, 3:], [1.0, -0.75, 0.25]) and np.allclose(pin[4, 3:], [1.0, 0.75, -0.25])
    assert p["chunk+1"].shape[0] == 257 and p["4096"].shape[0] == 4096 and p["single"].shape == (1, 6)


@pytest.mark.parametrize("case", CASES)
def test_exclusion_cap_on_the_gpu_tests_inputs(case):
    """From the reference alone: on the states, terrain and patterns tests/test_gpu_ray_cast.py casts, at most 2 % of
    the rays of any comparison are left out by the margins, the frames sit 0.6 .. 1.4 m above the ground under them,
    and triangles, the plane, the border's face and misses all occur."""
    hf = terrain()
    for align in ALIGNS:
        kinds = np.zeros(5, int)
        for pattern in ("lidar", "pinhole"):
            r = reference(case, N, 71, pattern, align)
            ex_d, ex_n = excluded_shares(r)
            assert ex_d <= rr.EXCLUDED_CAP and ex_n <= rr.EXCLUDED_CAP, (case, align, pattern, ex_d, ex_n)
            kinds += np.bincount(r.kind.ravel(), minlength=5)
            ground = surface_at(hf, r.frame_points[..., 0], r.frame_points[..., 1])[0]
            up = r.frame_points[..., 2] - ground
            assert 0.6 <= up.min() and up.max() <= 1.4, (case, up.min(), up.max())
        assert kinds[rr.MISS] > 10 and kinds[rr.PLANE] > 10 and kinds[rr.TRIANGLE] > 50 and kinds[rr.FACE] >= 2
    m, _frames, root, _dof = scenario(case)
    tilt = np.arccos(np.clip(1 - 2 * (root[:, 3] ** 2 + root[:, 4] ** 2), -1, 1))
    assert (tilt > 0.04).all() and (tilt < 0.16).all() and MAX_RANGE == 10.0
