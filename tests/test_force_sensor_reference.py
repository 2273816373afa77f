"""The float64 force sensor reference (tests/force_sensor_ref.py), pinned on the
CPU: the transport identity between two points, agreement of env and local
space under a known rotation, the torsion row's pure moment, and a known
answer for a box patch."""
import numpy as np

from tests.force_sensor_ref import box_patch_rows, transport, wrench_at


def _rows(rs, K=9):
    lam = rs.uniform(0.0, 0.2, K)
    d = rs.normal(size=(K, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    x = rs.normal(0, 0.3, (K, 3))
    tor = np.zeros(K, bool)
    tor[[3, 8]] = True
    return lam, d, x, tor


def _rot(rs):
    q = rs.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_transport_identity_between_two_points():
    rs = np.random.default_rng(0)
    for _ in range(20):
        lam, d, x, tor = _rows(rs)
        pa, pb = rs.normal(0, 0.5, 3), rs.normal(0, 0.5, 3)
        wa, wb = wrench_at(pa, lam, d, x, tor, 0.01), wrench_at(pb, lam, d, x, tor, 0.01)
        assert np.array_equal(wa[:3], wb[:3])
        assert np.abs(wb[3:] - wa[3:] - np.cross(pa - pb, wa[:3])).max() < 1e-12 * np.linalg.norm(wa[:3])
        assert np.abs(transport(wa, pa, pb) - wb).max() < 1e-12 * np.linalg.norm(wa[:3])


def test_env_and_local_space_agree_under_a_known_rotation():
    rs = np.random.default_rng(1)
    for _ in range(20):
        lam, d, x, tor = _rows(rs)
        p, R = rs.normal(0, 0.5, 3), _rot(rs)
        we, wl = wrench_at(p, lam, d, x, tor, 0.005), wrench_at(p, lam, d, x, tor, 0.005, R=R)
        assert np.abs(R @ wl[:3] - we[:3]).max() < 1e-12 and np.abs(R @ wl[3:] - we[3:]).max() < 1e-12
        # the same rows described in the link's axes give the local wrench directly
        wd = wrench_at(R.T @ p, lam, d @ R, x @ R, tor, 0.005)
        assert np.abs(wd - wl).max() < 1e-12
    # a quarter turn about z: world x is the link's -y
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    w = wrench_at([0, 0, 0], [0.01], [[1, 0, 0]], [[0, 0, 1]], [False], 0.01, R=Rz)
    assert np.allclose(w, [0, -1, 0, 1, 0, 0])


def test_torsion_row_is_a_pure_moment():
    w = wrench_at([0.3, -0.2, 0.1], [0.02], [[0, 0, 1]], [[5, 5, 5]], [True], 0.01)
    assert np.array_equal(w, [0, 0, 0, 0, 0, 2.0])   # no force, the same moment about every point


def test_box_patch_known_answer():
    """A level box of half extents (0.1, 0.075, 0.05) at height 0.05, 5 N on
    each corner: 20 N up through the centre, so no moment about the point
    under it and, about a point 4 cm ahead of it, n_y = +0.04 * 20."""
    h = 0.01
    pts, d, x, tor = box_patch_rows(np.eye(3), [2.0, 3.0, 0.05], (0.1, 0.075, 0.05))
    assert np.allclose(pts[:, 2], 0) and np.allclose(pts.mean(axis=0), [2, 3, 0])
    assert np.allclose(pts[:, :2] - [2, 3], [[-0.1, -0.075], [0.1, -0.075], [-0.1, 0.075], [0.1, 0.075]])
    lam = np.array([5, 5, 5, 5, 0, 0, 0]) * h
    assert np.allclose(wrench_at([2, 3, 0], lam, d, x, tor, h), [0, 0, 20, 0, 0, 0])
    assert np.allclose(wrench_at([2.04, 3, 0], lam, d, x, tor, h), [0, 0, 20, 0, 0.8, 0])
    # the centre of pressure (-n_y / f_z, n_x / f_z) relative to the sensor point
    w = wrench_at([2.04, 3.01, 0], np.array([8, 2, 8, 2, 0, 0, 0]) * h, d, x, tor, h)
    assert np.allclose([-w[4] / w[2], w[3] / w[2]], [(-0.1 * 16 + 0.1 * 4) / 20 - 0.04, -0.01])
    # the friction anchor: the corners weighted by their depth into the margin
    pts, d, x, tor = box_patch_rows(np.eye(3), [0, 0, 0.05], (0.1, 0.075, 0.05), margin=0.02,
                                    phi=[0.0, 0.01, 0.03, 0.02])
    assert np.allclose(x[4], (1.0 * pts[0] + 0.5 * pts[1]) / 1.5) and np.array_equal(x[4], x[6])
