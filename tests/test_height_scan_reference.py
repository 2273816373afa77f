"""The float64 reference of the height scan (tests/height_scan_ref.py) pinned
without a GPU: known answers worked by hand on a literal 3 x 4 heightfield, the
yaw rule against an explicit quaternion product, the relative clamp, the
pattern's order, and the exclusion cap of tests/test_gpu_height_scan.py on that
file's own inputs.

The field (raw samples; hs = 0.5, vs = 0.1, origin (1, -2)), vertex (i, j) at
(1 + 0.5 i, -2 + 0.5 j, 0.1 H[i][j]):
        j = 0   1   2   3
  i = 0     1   2   3   4
  i = 1     5   6  -8   8
  i = 2     9  10  11  12
Cell (0, 1) has the corners h00 = 0.2, h01 = 0.3 (j + 1), h10 = 0.6 (i + 1),
h11 = -0.8:
  lower triangle, fu = 0.75 >= fv = 0.25: gx = h10 - h00 = 0.4, gy = h11 - h10 =
    -1.4, H = 0.2 + 0.3 - 0.35 = 0.15, slopes (0.8, -2.8), n = (-0.8, 2.8, 1) /
    sqrt(9.48)
  upper triangle, fu = 0.1 < fv = 0.9: gx = h11 - h01 = -1.1, gy = h01 - h00 =
    0.1, H = 0.2 - 0.11 + 0.09 = 0.18, slopes (-2.2, 0.2), n = (2.2, -0.2, 1) /
    sqrt(5.88)
  upper triangle, fu = 0.25 < fv = 0.5: H = 0.2 - 0.275 + 0.05 = -0.025: the
    plane wins, h = 0, n = e_z; the cell rule shows 0.1 min(2, -8) = -0.8
Vertex (1, 1) at (1.5, -1.5): h = 0.6; it is the (0, 0) corner of cell (1, 1),
lower triangle: gx = 1.0 - 0.6 = 0.4, gy = 1.1 - 1.0 = 0.1, n = (-0.8, -0.2, 1)
/ sqrt(1.68)."""
import numpy as np
import pytest

from tests import physics_models as pm
from tests.height_scan_ref import (EXCLUDED_CAP, MARGIN_CELLS, Heightfield, cell_at, height_scan_ref,
                                   reference_pattern, sample_points, surface_at, yaw_matrix)
from tests.jacobian_ref import quat_R

HF = Heightfield(np.array([[1, 2, 3, 4], [5, 6, -8, 8], [9, 10, 11, 12]], np.float32), 0.5, 0.1, 1.0, -2.0)


def xy(i, j, fu, fv):
    return 1.0 + 0.5 * (i + fu), -2.0 + 0.5 * (j + fv)


def test_both_triangles_of_a_cell():
    h, n, _mb, _mn = surface_at(HF, *xy(0, 1, 0.75, 0.25))
    assert h == pytest.approx(0.15, abs=1e-7)
    assert np.allclose(n, np.array([-0.8, 2.8, 1.0]) / np.sqrt(9.48), atol=1e-7)
    h, n, _mb, _mn = surface_at(HF, *xy(0, 1, 0.1, 0.9))
    assert h == pytest.approx(0.18, abs=1e-7)
    assert np.allclose(n, np.array([2.2, -0.2, 1.0]) / np.sqrt(5.88), atol=1e-7)
    assert abs(np.linalg.norm(n) - 1.0) < 1e-15
    # the two rules agree on the diagonal itself, the surface is continuous: cell (1, 1), corners 0.6, -0.8 (j + 1),
    # 1.0 (i + 1), 1.1; lower 0.6 + 0.5 0.4 + 0.5 0.1 = 0.85, upper 0.6 + 0.5 1.9 - 0.5 1.4 = 0.85
    a = surface_at(HF, *xy(1, 1, 0.5, 0.5 + 1e-12))[0]
    b = surface_at(HF, *xy(1, 1, 0.5 + 1e-12, 0.5))[0]
    assert abs(a - b) < 1e-11 and a == pytest.approx(0.85, abs=1e-7)


def test_a_vertex():
    h, n, _mb, mn = surface_at(HF, 1.5, -1.5)
    assert h == pytest.approx(0.6, abs=1e-7)
    assert np.allclose(n, np.array([-0.8, -0.2, 1.0]) / np.sqrt(1.68), atol=1e-7)
    assert mn == 0.0                                # a vertex lies on the cell lines: the normal jumps there
    hc, mc = cell_at(HF, 1.5, -1.5)
    assert hc == pytest.approx(0.1 * min(6, 11), abs=1e-7) and mc == 0.0


def test_a_negative_patch_the_plane_wins_and_the_cell_rule_shows_the_raw_value():
    x, y = xy(0, 1, 0.25, 0.5)
    h, n, _mb, _mn = surface_at(HF, x, y)
    assert h == 0.0 and np.array_equal(n, [0.0, 0.0, 1.0])
    hc, _m = cell_at(HF, x, y)
    assert hc == pytest.approx(-0.8, abs=1e-7)
    # the cell rule is constant over the cell, the lower of the (i, j) and (i + 1, j + 1) corners
    assert cell_at(HF, *xy(0, 0, 0.9, 0.1))[0] == pytest.approx(0.1 * min(1, 6), abs=1e-7)
    assert cell_at(HF, *xy(1, 2, 0.3, 0.6))[0] == pytest.approx(0.1 * min(-8, 12), abs=1e-7)


def test_off_grid_points():
    # below the grid in x: the plane in SURFACE, the border cell in CELL
    x, y = 0.9, xy(0, 0, 0.0, 0.25)[1]
    h, n, mb, _mn = surface_at(HF, x, y)
    assert h == 0.0 and np.array_equal(n, [0.0, 0.0, 1.0]) and mb == pytest.approx(0.2)     # 0.1 m = 0.2 cells out
    assert cell_at(HF, x, y)[0] == pytest.approx(0.1 * min(1, 6), abs=1e-7)
    # far beyond the far corner: i = rows - 2, j = cols - 2
    h, n, _mb, _mn = surface_at(HF, 5.0, 10.0)
    assert h == 0.0 and np.array_equal(n, [0.0, 0.0, 1.0])
    hc, mc = cell_at(HF, 5.0, 10.0)
    assert hc == pytest.approx(0.1 * min(-8, 12), abs=1e-7) and mc > 1.0
    # just inside the far border the surface is the mesh again
    assert surface_at(HF, 2.0 - 1e-9, -0.5 - 1e-9)[0] == pytest.approx(1.2, abs=1e-6)
    # without a heightfield
    h, n, mb, mn = surface_at(None, np.array([0.3, 7.0]), np.array([0.0, -2.0]))
    assert not h.any() and np.array_equal(n, [[0, 0, 1], [0, 0, 1]]) and np.isinf(mb).all() and np.isinf(mn).all()
    assert not cell_at(None, np.array([0.3]), np.array([0.0]))[0].any()


def test_margins():
    # cell rule: 0.1 cells from the line u = 1; the lines u = 0 and u = rows - 1 do not count (the index is clamped)
    assert cell_at(HF, *xy(0, 1, 0.9, 0.5))[1] == pytest.approx(0.1)
    assert cell_at(HF, *xy(0, 0, 0.05, 0.5))[1] == pytest.approx(0.5)        # v = 0.5: half a cell from v = 1
    # normals: the cell lines (cell (1, 2), lower triangle, H = -0.8 + 1.9 fu + 0.1 fv = 0.96: the zero crossing is
    # half a cell away, the diagonal 0.28)
    assert surface_at(HF, *xy(1, 2, 0.9, 0.5))[3] == pytest.approx(0.1)
    # normals: the diagonal, in cells along its normal
    assert surface_at(HF, *xy(0, 0, 0.5, 0.46))[3] == pytest.approx(0.04 / np.sqrt(2.0))
    # normals: the H = 0 crossing, |H| / |grad H| with the gradient per cell
    x, y = xy(0, 1, 0.25, 0.5)
    assert surface_at(HF, x, y)[3] == pytest.approx(0.025 / np.hypot(1.1, 0.1), rel=1e-5)
    # surface heights: only the border
    assert surface_at(HF, x, y)[2] == pytest.approx(0.25)


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def test_yaw_rule_against_an_explicit_quaternion_product():
    """quat_apply_yaw: the quaternion with x and y zeroed, normalised, applied as q v q^-1."""
    rs = np.random.default_rng(3)
    for _ in range(50):
        q = rs.normal(0, 1, 4)
        q /= np.linalg.norm(q)
        qy = np.array([0.0, 0.0, q[2], q[3]])
        if np.linalg.norm(qy) < 1e-3:
            continue
        qy /= np.linalg.norm(qy)
        a, b = rs.uniform(-1, 1, 2)
        v = _quat_mul(_quat_mul(qy, np.array([a, b, 0.0, 0.0])), qy * np.array([-1, -1, -1, 1.0]))
        assert abs(v[2]) < 1e-15 and abs(v[3]) < 1e-15
        assert np.allclose(yaw_matrix(quat_R(q)) @ np.array([a, b]), v[:2], atol=1e-13)
    # w = z = 0: no heading, the identity
    assert np.array_equal(yaw_matrix(quat_R([1.0, 0.0, 0.0, 0.0])), np.eye(2))
    assert np.array_equal(yaw_matrix(quat_R([0.0, 1.0, 0.0, 0.0])), np.eye(2))
    # a pure yaw of 90 degrees turns (1, 0) into (0, 1)
    s = np.sqrt(0.5)
    assert np.allclose(yaw_matrix(quat_R([0, 0, s, s])) @ np.array([1.0, 0.0]), [0.0, 1.0], atol=1e-15)


def test_alignments_on_a_tilted_body():
    R = quat_R(np.array([0.3, -0.2, 0.5, 0.79]) / np.linalg.norm([0.3, -0.2, 0.5, 0.79]))
    p = np.array([[[2.0, -1.0, 0.7]]])
    pts = np.array([[0.4, 0.0], [0.0, -0.3]], np.float32)
    w = sample_points(p, R[None, None], pts, "world")[0, 0]
    assert np.allclose(w, [[2.4, -1.0], [2.0, -1.3]], atol=1e-7)
    l = sample_points(p, R[None, None], pts, "link")[0, 0]
    assert np.allclose(l[0], p[0, 0, :2] + np.float64(pts[0, 0]) * R[:2, 0]) and \
        np.allclose(l[1], p[0, 0, :2] + np.float64(pts[1, 1]) * R[:2, 1])
    y = sample_points(p, R[None, None], pts, "yaw")[0, 0]
    assert np.allclose(np.linalg.norm(y - p[0, 0, :2], axis=1), [0.4, 0.3], atol=1e-7)      # a rotation keeps lengths
    assert np.linalg.norm(l[0] - p[0, 0, :2]) < 0.4 - 1e-3                                  # the projection shortens


def test_relative_clamp_and_frame_point_on_a_free_body():
    m = pm.free_body()
    root = np.zeros((3, 13), np.float32)
    root[:, 6] = 1.0
    root[:, :3] = [[1.3, -1.8, 0.9], [1.3, -1.8, 3.0], [1.3, -1.8, -2.0]]
    dof = np.zeros((0, 2), np.float32)
    frames = [(0, (0.075, 0.0625, 0.25))]         # p_f = root + offset: (1.375, -1.7375, z + 0.25) -- cell (0, 0)
    pts = np.array([[0.0, 0.0]], np.float32)
    r = height_scan_ref(m, root, dof, frames, pts, HF, "surface", "world")
    assert np.allclose(r.frame_points[:, 0], root[:, :3].astype(np.float64) + [0.075, 0.0625, 0.25], atol=1e-7)
    # cell (0, 0) is the plane H = 0.1 + 0.4 fu + 0.1 fv: fu = 0.75, fv = 0.525
    h = 0.1 + 0.4 * 0.75 + 0.1 * 0.525
    assert np.allclose(r.heights[:, 0, 0], h, atol=1e-6) and r.raw is r.heights
    rel = dict(bias=0.5, lo=-1.0, hi=1.0, scale=5.0)
    r = height_scan_ref(m, root, dof, frames, pts, HF, "surface", "world", relative=rel)
    assert np.allclose(r.heights[:, 0, 0], [5.0 * (0.9 + 0.25 - 0.5 - h), 5.0, -5.0], atol=1e-5)
    assert np.allclose(r.raw[:, 0, 0], h, atol=1e-6)
    r = height_scan_ref(m, root, dof, frames, pts, HF, "cell", "world", relative=rel)
    assert np.allclose(r.heights[:, 0, 0], [5.0 * (0.9 + 0.25 - 0.5 - 0.1), 5.0, -5.0], atol=1e-5)
    assert r.normals is None and r.margin_normals is None


def test_reference_pattern_is_the_reference_order():
    p = reference_pattern()
    assert p.shape == (140, 2) and p.dtype == np.float32
    assert np.allclose(p[0], [-0.8, -0.5]) and np.allclose(p[1], [-0.8, -0.4]) and np.allclose(p[10], [-0.7, -0.5])
    assert np.allclose(p[-1], [0.8, 0.5]) and not (np.abs(p[:, 0]) < 0.15).any() and not (np.abs(p[:, 1]) < 0.05).any()
    torch = pytest.importorskip("torch")
    y = 0.1 * torch.tensor([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], dtype=torch.float32)
    x = 0.1 * torch.tensor([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8], dtype=torch.float32)
    gx, gy = torch.meshgrid(x, y, indexing="ij")
    assert np.array_equal(p, torch.stack([gx.flatten(), gy.flatten()], 1).numpy())


@pytest.mark.parametrize("case", ["thormang", "gogoro", "jit_walker", "kat_free"])
def test_exclusion_cap_on_the_gpu_tests_inputs(case):
    """From the reference alone: on the states, terrain and patterns tests/test_gpu_height_scan.py scans, at most 2 %
    of the samples of any mode lie within MARGIN_CELLS of a discontinuity (expected at most 6e-3: three line families
    at 2e-3 each)."""
    from tests.test_gpu_height_scan import modes, scenario, terrain
    hf = terrain()
    for n, seed in ((5, 61), (1, 62)):
        m, frames, root, dof = scenario(case, n, seed)
        for pts in (reference_pattern(), np.array([[0.3, -0.2]], np.float32)):
            if pts.shape[0] == 1 and n == 1:
                continue
            for key, surface, align, _normals, relative, _o in modes():
                r = height_scan_ref(m, root, dof, frames, pts, hf, surface, align, relative)
                share = float((r.margin < MARGIN_CELLS).mean())
                assert share <= EXCLUDED_CAP, (case, n, key, share)
                if r.margin_normals is not None:
                    share = float((r.margin_normals < MARGIN_CELLS).mean())
                    assert share <= EXCLUDED_CAP, (case, n, key, share)
                if pts.shape[0] > 1 and n > 1 and surface == "surface" and relative is None:
                    on = np.isfinite(r.margin_normals) & (r.normals[..., 2] < 1.0)
                    assert 0.5 < on.mean() < 1.0 and (r.heights == 0.0).any()       # most on the mesh, some not
