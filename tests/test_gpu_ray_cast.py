"""The ray cast on the GPU (tg_ray_cast, Sim.ray_cast) against the float64
reference (tests/ray_cast_ref.py, pinned by tests/test_ray_cast_reference.py).

Sims of five envs and of one.  Every env stands nearly upright -- a random
heading, a tilt of 0.05 .. 0.15 rad about a random horizontal axis, joint
angles within +-0.15 rad -- with its frames 0.6 .. 1.4 m above the ground under
them (frame offsets along the link's vertical bring the head and a foot of the
humanoid into that band; asserted from the reference).  Env 1 stands at FAR,
tens of metres from env 0 and still on the grid; env 2 stands at EDGE, 0.4 m
outside the grid's x = -7 border where the field is about 0.3 m high, low and
facing the border, so that some of its rays enter the terrain through the
border's vertical face.  The heightfield is height_scan's: 200 x 168 samples,
hs = 0.25, vs = 0.005, origin (-7, -4.5), smooth, a few decimetres high, with
negative patches.  Patterns: a lidar of 16 azimuths (offset 3 degrees) x the
elevations -50, -30, -15, -7, -2, +8 degrees (96 rays; F R = 288 with three
frames, no multiple of 64), a 16 x 12 pinhole image pitched down 0.45 rad, a
single ray, 257 rays (one more than the kernel's chunk of 256 samples) and 4096
rays on one env and one frame.  Every output is filled with NaN before each
call.

Exclusion.  A ray is left out when its graze clearance or its distance to
max_range is under CLEAR = 1 mm, or it lands flatter than COS_MIN = 0.05; for
the normals also when the plane and the terrain candidates are within CLEAR or
the hit within MARGIN_CELLS = 1e-3 cells of a cell line or diagonal
(ray_cast_ref's margins).  CLEAR is asserted below to be at least 8 fp32 ulps
of the largest coordinate divided by COS_MIN.  At most 2 % of a case may be left
out (asserted here and, from the reference alone, in
tests/test_ray_cast_reference.py).

Tolerance.  max |got - ref| / max_range for dist and max |got - ref| for the
normals were measured per case on the MI355X on this file's first run
(RAY_MEASURED below; the worst over every comparison the file makes for the
case).  Asserted: 4 x the measured value, under the project's hard cap of 1e-4.
The expected error is the fp32 rounding of a 40 m coordinate, 4e-6 m, divided by
the incidence cosine.  Worst measured: dist 8.7e-7 of max_range (thormang,
after a step of the call sequence), normals 6.3e-8; at most 1.7 % of a
comparison's rays were left out.  The exact checks take no tolerance."""
import functools

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests import ray_cast_ref as rr
from tests.height_scan_ref import Heightfield, frame_poses, smooth_heightfield, surface_at
from tests.jacobian_ref import quat_R
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

N = 5
FAR = (40.07, 30.11)        # env 1
EDGE_X = -7.4               # env 2: 0.4 m outside the border x = -7; its y is where the border is highest (edge_xy)
CASES = ["thormang", "gogoro", "jit_walker", "kat_free"]
ALIGNS = ["link", "yaw", "world"]
MAX_RANGE = 10.0
# max |got - ref| / max_range of dist and max |got - ref| of the normals, measured on the MI355X: the worst over every
# comparison this file makes for the case
RAY_MEASURED = {
    #              dist    normals
    "thormang":    [8.7e-7, 6.3e-8],
    "gogoro":      [3.9e-7, 6.2e-8],
    "jit_walker":  [7.1e-7, 5.9e-8],
    "kat_free":    [4.9e-7, 5.9e-8],
    "gogoro_task": [3.4e-7, None],                     # (the task tests compare the depth only)
}
HARD_CAP = 1e-4
assert all(4 * v <= HARD_CAP for row in RAY_MEASURED.values() for v in row if v is not None)


def tolerance(case, output):
    return 4 * dict(zip(("dist", "normals"), RAY_MEASURED[case]))[output]


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return {"jit_walker": pm.jit_walker, "kat_free": pm.free_body}.get(name, lambda: load_model(name))()


def terrain(seed=7):
    return smooth_heightfield(200, 168, np.random.default_rng(seed))


@functools.lru_cache(maxsize=None)
def edge_xy():
    """Env 2's place: EDGE_X, and the y (off the lattice) at which the border x = -7 is highest."""
    hf = terrain()
    j = int(np.argmax(hf.heights[0, 20:-20])) + 20
    assert float(hf.vs) * hf.heights[0, j] > 0.25
    return EDGE_X, float(hf.oy) + (j + 0.37) * float(hf.hs)


def lidar():
    return rr.lidar_pattern(np.deg2rad(3.0 + 22.5 * np.arange(16)), np.deg2rad([-50.0, -30.0, -15.0, -7.0, -2.0, 8.0]))


def pitched(rays, pitch):
    """The pattern turned nose-down by ``pitch`` about its y axis."""
    c, s = np.cos(pitch), np.sin(pitch)
    Ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    out = np.asarray(rays, np.float64).copy()
    out[:, :3], out[:, 3:] = out[:, :3] @ Ry.T, out[:, 3:] @ Ry.T
    return out.astype(np.float32)


def patterns():
    """name -> rays [R, 6] float32."""
    return {
        "lidar": lidar(),
        "pinhole": pitched(rr.pinhole_pattern(16, 12, np.deg2rad(87.0)), 0.45),
        "single": np.array([[0.0, 0.0, 0.0, 0.6, 0.1, -0.8]], np.float32),
        "chunk+1": rr.lidar_pattern(np.deg2rad(1.0 + 360.0 / 257 * np.arange(257)), np.deg2rad([-20.0])),
        "4096": pitched(rr.pinhole_pattern(64, 64, np.deg2rad(87.0)), 0.6),
    }


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def case_links(case, m):
    """(link index, nominal height of the frame above the root origin) of a case's frames."""
    if case == "thormang":
        from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
        return [(0, 0.0), (m.link_index("lidar_link"), 0.15), (walk_feet_indices(m)[0], -0.1)]
    if case == "gogoro":
        return [(m.link_index("realsense_link"), 0.1)]
    if case == "jit_walker":
        return [(0, 0.0), (m.num_bodies - 1, -0.1)]
    return [(0, 0.2), (0, 0.0)]                     # kat_free: one link in two frames


@functools.lru_cache(maxsize=None)
def scenario(case, n=N, seed=71):
    """(model, frames, root, dof) of a case: no GPU needed (the reference test reads it too).  ``frames``: (link,
    offset) pairs, the offset along the link's vertical at the zero pose so that the frame sits ``nominal`` above the
    root origin there."""
    m = _model(case)
    rs = np.random.default_rng(seed)
    hf = terrain()
    root0 = np.zeros((1, 13), np.float32)
    root0[0, 6] = 1.0
    dof0 = np.zeros((m.num_dof, 2), np.float32)
    links = case_links(case, m)
    p0, R0 = frame_poses(m, root0, dof0, [(l, (0.0, 0.0, 0.0)) for l, _h in links])
    frames = []
    for f, (l, nominal) in enumerate(links):
        off = R0[0, f].T @ np.array([0.02 * f, -0.01 * f, nominal - p0[0, f, 2]])
        frames.append((l, tuple(float(np.float32(x)) for x in off)))
    root = np.zeros((n, 13), np.float32)
    dof = np.zeros((n * m.num_dof, 2), np.float32)
    dof[:, 0] = rs.uniform(-0.15, 0.15, n * m.num_dof)
    xy = np.stack([rs.uniform(-4.0, 30.0, n), rs.uniform(-2.0, 30.0, n)], 1)
    yaw = rs.uniform(-np.pi, np.pi, n)
    base = np.full(n, 1.0)
    if n > 2:
        xy[1], xy[2] = FAR, edge_xy()
        yaw[2], base[2] = 0.1, 0.75                  # env 2 faces the border from 0.4 m, low
    for e in range(n):
        ax, ang = rs.uniform(0, 2 * np.pi), rs.uniform(0.05, 0.15)
        tilt = np.array([np.cos(ax) * np.sin(ang / 2), np.sin(ax) * np.sin(ang / 2), 0.0, np.cos(ang / 2)])
        q = _quat_mul(np.array([0.0, 0.0, np.sin(yaw[e] / 2), np.cos(yaw[e] / 2)]), tilt)
        ground = float(surface_at(hf, xy[e, 0], xy[e, 1])[0])
        root[e, :2], root[e, 2], root[e, 3:7] = xy[e], ground + base[e], q / np.linalg.norm(q)
    return m, tuple(frames), root, dof


@functools.lru_cache(maxsize=None)
def reference(case, n, seed, pattern, align, with_terrain=True, max_range=MAX_RANGE):
    m, frames, root, dof = scenario(case, n, seed)
    return rr.ray_cast_ref(m, root, dof, list(frames), patterns()[pattern], terrain() if with_terrain else None, align,
                           max_range)


def excluded_shares(ref):
    return float(1.0 - rr.keep_dist(ref).mean()), float(1.0 - rr.keep_normals(ref).mean())


def test_clear_covers_the_rounding_of_the_env_placement():
    hf = terrain()
    reach = max(abs(FAR[0]), abs(FAR[1]), abs(EDGE_X)) + MAX_RANGE + 2.0     # the farthest point a kept ray reaches
    assert rr.CLEAR >= 8 * float(np.spacing(np.float32(reach))) / rr.COS_MIN
    assert hf.heights.shape[0] != hf.heights.shape[1] and float(hf.vs) != 1.0 and float(hf.hs) == 0.25
    z = float(hf.vs) * hf.heights
    assert z.min() < -0.1 and 0.2 < z.max() < 0.5
    u, v = (FAR[0] - float(hf.ox)) / float(hf.hs), (FAR[1] - float(hf.oy)) / float(hf.hs)
    assert 0 < u < hf.heights.shape[0] - 1 and 0 < v < hf.heights.shape[1] - 1
    x, y = edge_xy()
    assert x < float(hf.ox) and float(hf.oy) < y < float(hf.oy) + (hf.heights.shape[1] - 1) * float(hf.hs)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")


class Case:
    """A sim of ``n`` envs in the test state on the test terrain."""

    def __init__(self, case, n=N, seed=71):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.case, self.n, self.seed = case, n, seed
        self.m, frames, self.root, self.dof = scenario(case, n, seed)
        self.frames = list(frames)
        m = self.m
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        s.refresh()
        self.set_terrain(terrain())
        self.F = len(self.frames)
        self.cframes = [s.contact_frame(l, o) for l, o in self.frames]
        self.rays = {k: torch.from_numpy(v).cuda() for k, v in patterns().items()}

    def set_terrain(self, hf):
        self.hf = hf
        if hf is None:
            self.s.set_heightfield(None)
        else:
            self.s.set_heightfield(hf.heights, float(hf.hs), float(hf.vs), float(hf.ox), float(hf.oy))

    def call(self, pattern, align, max_range=MAX_RANGE, want=("dist", "normals"), frames=None):
        """One call of the C function on NaN-filled outputs; (dist, normals) as numpy, all NaN when not asked for."""
        from thormang_isaacgym_amd._lib import lib
        rays = self.rays[pattern] if isinstance(pattern, str) else pattern
        cf = self.cframes if frames is None else frames
        R = rays.shape[0]
        d, nn = _nan(self.n, len(cf), R), _nan(self.n, len(cf), R, 3)
        rp = abi.tg_ray_params()
        rp.align = {"link": abi.TG_RAY_LINK, "yaw": abi.TG_RAY_YAW, "world": abi.TG_RAY_WORLD}[align]
        rp.max_range = max_range
        arr = (abi.tg_contact_frame * len(cf))(*cf)
        rc = lib().tg_ray_cast(self.s.handle, arr, len(cf), rays.data_ptr(), R, rp,
                               d.data_ptr() if "dist" in want else None, nn.data_ptr() if "normals" in want else None)
        assert rc == 0, lib().tg_last_error()
        torch.cuda.synchronize()
        return d.cpu().numpy(), nn.cpu().numpy()

    def reference(self, pattern, align, root=None, dof=None, max_range=MAX_RANGE):
        if root is None and self.hf is not None and isinstance(pattern, str):
            return reference(self.case, self.n, self.seed, pattern, align, True, max_range)
        rays = patterns()[pattern] if isinstance(pattern, str) else pattern
        return rr.ray_cast_ref(self.m, self.root if root is None else root, self.dof if dof is None else dof,
                               self.frames, rays, self.hf, align, max_range)

    def check(self, key, got, ref, max_range=MAX_RANGE, case=None):
        """Compares one call with its reference over the rays kept; prints and returns the figures."""
        d, nn = got
        assert d.dtype == np.float32 and not np.isnan(d).any() and not np.isnan(nn).any()      # every element written
        kd, kn = rr.keep_dist(ref), rr.keep_normals(ref)
        ex_d, ex_n = excluded_shares(ref)
        hit, hit_ref = d < np.float32(max_range), ref.dist < max_range
        fig = {"dist": float((np.abs(d - ref.dist)[kd] / max_range).max()),
               "normals": float(np.abs(nn - ref.normals)[kn].max()),
               "excluded": ex_d, "excluded_normals": ex_n}
        print({"case": self.case, "n": self.n, "call": key, **fig})
        assert ex_d <= rr.EXCLUDED_CAP and ex_n <= rr.EXCLUDED_CAP, (key, fig)
        assert np.array_equal(hit[kd], hit_ref[kd]), key                                   # hit or miss agrees
        assert np.array_equal(d[~hit], np.full((~hit).sum(), max_range, np.float32)), key  # misses: max_range exactly
        assert not nn[~hit].any(), key                                                     # and a zero normal
        assert float(np.abs(np.linalg.norm(nn[hit], axis=-1) - 1.0).max(initial=0.0)) <= 1e-6, key
        assert fig["dist"] <= tolerance(case or self.case, "dist"), (key, fig)
        assert fig["normals"] <= tolerance(case or self.case, "normals"), (key, fig)
        return fig


_cases = {}


def shared(case, n=N, seed=71):
    if (case, n) not in _cases:
        _cases[case, n] = Case(case, n, seed)
    return _cases[case, n]


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("case", CASES)
def test_outputs_match_the_reference(case, align):
    c = shared(case)
    kinds = np.zeros(5, int)
    for pattern in ("lidar", "pinhole"):
        ref = c.reference(pattern, align)
        c.check(f"{pattern}/{align}", c.call(pattern, align), ref)
        kinds += np.bincount(ref.kind.ravel(), minlength=5)
        if c.n > 2:
            assert (ref.kind[[0, 1, 3, 4]] != rr.FACE).all()                # (only env 2 stands at the border)
    print({"case": case, "align": align, "miss plane triangle face inside": kinds.tolist()})
    # triangles, the plane, the border's face (env 2) and misses all occur
    assert kinds[rr.MISS] > 10 and kinds[rr.PLANE] > 10 and kinds[rr.TRIANGLE] > 50 and kinds[rr.FACE] >= 2


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_dist_alone_and_normals_alone(case):
    c = shared(case)
    for align in ALIGNS:
        both = c.call("lidar", align)
        d, n0 = c.call("lidar", align, want=("dist",))
        assert np.array_equal(d.view(np.uint32), both[0].view(np.uint32)) and np.isnan(n0).all()
        d0, nn = c.call("lidar", align, want=("normals",))
        assert np.array_equal(nn.view(np.uint32), both[1].view(np.uint32)) and np.isnan(d0).all()


@pytest.mark.parametrize("case", ["thormang", "gogoro", "kat_free"])
def test_one_env(case):
    c = shared(case, 1, 72)
    for align in ALIGNS:
        c.check(f"lidar/{align}", c.call("lidar", align), c.reference("lidar", align))


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_single_ray_pattern(case):
    c = shared(case)
    for align in ALIGNS:
        got = c.call("single", align)
        assert got[0].shape == (c.n, c.F, 1)
        c.check(f"single/{align}", got, c.reference("single", align))


@pytest.mark.parametrize("case,n", [("gogoro", 5), ("thormang", 1)])
def test_one_ray_more_than_a_chunk(case, n):
    """257 rays: F R = 257 takes two blocks per env, 771 four (the last chunk of three samples)."""
    c = shared(case, n, 71 if n == N else 72)
    assert patterns()["chunk+1"].shape[0] == 256 + 1
    c.check("chunk+1/link", c.call("chunk+1", "link"), c.reference("chunk+1", "link"))


def test_4096_rays_on_one_env_and_one_frame():
    c = shared("gogoro", 1, 72)
    assert patterns()["4096"].shape[0] == abi.TG_RAY_MAX_RAYS and c.F == 1
    c.check("4096/link", c.call("4096", "link"), c.reference("4096", "link"))


def test_runtime_loaded_model():
    """jit_walker is compiled at run time (tg_model_jit): the call works, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = shared("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()
    c.check("lidar/link", c.call("lidar", "link"), c.reference("lidar", "link"))


# ------------------------------------------------------------------ exact checks

PLATEAU = Heightfield(np.full((5, 4), 1.0, np.float32), np.float32(0.25), np.float32(0.5), np.float32(2.0),
                      np.float32(4.0))         # x in [2, 3], y in [4, 4.75], top at z = 0.5
PLATEAU_ROOT = (2.5, 4.25, 0.0)
PLATEAU_RANGE = 4.0
NAN = float("nan")
# (start offset, direction) about PLATEAU_ROOT in world axes -> (dist, normal)
PLATEAU_TABLE = [
    ((0, 0, 2), (0, 0, -1), 1.5, (0, 0, 1)),                  # down onto the top from z = 2
    ((-1.5, 0, 2), (0, 0, -1), 2.0, (0, 0, 1)),               # down beside the plateau
    ((-1.5, 0, 0.25), (1, 0, 0), 1.0, (-1, 0, 0)),            # horizontal +x at z = 0.25 from 1 m outside
    ((0, -1.25, 0.25), (0, 1, 0), 1.0, (0, -1, 0)),           # the same along +y
    ((-1.5, 0, 0.75), (1, 0, 0), PLATEAU_RANGE, (0, 0, 0)),   # horizontal above the top: a miss
    ((0, 0, 1), (0.25, 0.125, 1), PLATEAU_RANGE, (0, 0, 0)),  # upward: a miss
    ((0, 0, 0.25), (1, 0, 0.5), 0.0, (0, 0, 1)),              # started under the plateau's top
    ((-1.5, 0, -1), (0, 0, 1), 0.0, (0, 0, 1)),               # started at z = -1
    ((-1.0, 0, 1.5), (1, 0, -1), 1.0, (0, 0, 1)),             # d = (1, 0, -1) from 1 m above the top
    ((0, 0, 2), (0, 0, -2), 0.75, (0, 0, 1)),                 # d = (0, 0, -2): t is the parameter, not the range
    ((0, 0, 1), (1, 0, -0.5), 2.0, (0, 0, 1)),                # leaves over the top edge, lands on the plane beyond
    ((-1.5, 0, 4.0 + 2.0 ** -10), (0, 0, -1), PLATEAU_RANGE, (0, 0, 0)),     # a hit just beyond max_range: a miss
    ((0, 0, 2), (0, 0, 0), PLATEAU_RANGE, (0, 0, 0)),         # zero direction
    ((0, 0, 2), (0, NAN, -1), PLATEAU_RANGE, (0, 0, 0)),      # NaN direction
]


def plateau_rays():
    return np.array([list(s) + list(d) for s, d, _t, _n in PLATEAU_TABLE], np.float32)


def _kat_sim(n, roots):
    from thormang_isaacgym_amd.sim import Sim
    m = _model("kat_free")
    s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
    root = np.zeros((n, 13), np.float32)
    root[:, 6] = 1.0
    root[:, :3] = roots
    s.root_state.copy_(torch.from_numpy(root))
    s.refresh()
    return m, s, root


def test_plateau_table_is_exact():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    _m, s, _root = _kat_sim(2, [PLATEAU_ROOT, PLATEAU_ROOT])
    hf = PLATEAU
    s.set_heightfield(hf.heights, float(hf.hs), float(hf.vs), float(hf.ox), float(hf.oy))
    rays = torch.from_numpy(plateau_rays()).cuda()
    for align in ALIGNS:                                   # an identity rotation: every alignment is the identity
        d, nn = _nan(2, 1, len(PLATEAU_TABLE)), _nan(2, 1, len(PLATEAU_TABLE), 3)
        s.ray_cast([s.contact_frame(0)], rays, align=align, max_range=PLATEAU_RANGE, normals=True, out=d,
                   out_normals=nn)
        torch.cuda.synchronize()
        d, nn = d.cpu().numpy(), nn.cpu().numpy()
        want_d = np.array([t for _s, _d, t, _n in PLATEAU_TABLE], np.float32)
        want_n = np.array([n for _s, _d, _t, n in PLATEAU_TABLE], np.float32)
        for e in range(2):
            assert np.array_equal(d[e, 0].view(np.uint32), want_d.view(np.uint32)), (align, d[e, 0], want_d)
            assert np.array_equal(nn[e, 0], want_n), (align, nn[e, 0])


RAMP = Heightfield((40.0 + 8.0 * np.arange(9)[:, None] + 4.0 * np.arange(7)[None, :]).astype(np.float32),
                   np.float32(0.25), np.float32(0.0078125), np.float32(1.0), np.float32(-2.0))
# H = 0.3125 + 0.25 (x - 1) + 0.125 (y + 2) on x in [1, 3], y in [-2, -0.5]: both triangles of every cell coplanar


def ramp_rays():
    """Rays from (2, -1.25, 0) + s about the middle of the ramp, each landing on the grid: along a cell line, along
    a cell diagonal, parallel to each axis, vertical, and two general ones."""
    return np.array([
        [-0.75, 0.0, 2.0, 1.0, 0.0, -1.0],          # along the cell line y = -1.25
        [0.0, -0.5, 2.0, 0.0, 1.0, -2.0],           # along the cell line x = 2
        [-0.75, -0.5, 2.0, 1.0, 1.0, -2.0],         # along the diagonals of the cells (1 + k, 1 + k)
        [-0.7, 0.1, 1.5, 1.0, 0.0, -1.5],           # parallel to x
        [0.3, -0.6, 1.5, 0.0, 1.0, -1.5],           # parallel to y
        [0.1, 0.05, 2.0, 0.0, 0.0, -1.0],           # vertical
        [0.25, 0.0, 2.0, 0.0, 0.0, -3.0],           # vertical on a cell line
        [-0.6, 0.4, 1.7, 0.9, -0.7, -2.0],
        [0.7, -0.5, 1.2, -1.3, 0.8, -1.0],
    ], np.float32)


def ramp_analytic(rays, root=(2.0, -1.25, 0.0)):
    o = np.asarray(root, np.float64) + rays[:, :3].astype(np.float64)
    d = rays[:, 3:].astype(np.float64)
    g = np.array([0.25, 0.125])
    h0 = 0.3125 - 0.25 * 1.0 + 0.125 * 2.0
    # z = h0 + g . (x, y): o.z + t d.z = h0 + g . (o.xy + t d.xy)
    return (h0 + o[:, :2] @ g - o[:, 2]) / (d[:, 2] - d[:, :2] @ g)


def test_ramp_rays_along_cell_lines_and_diagonals_match_the_analytic_value():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    _m, s, _root = _kat_sim(1, [(2.0, -1.25, 0.0)])
    hf = RAMP
    s.set_heightfield(hf.heights, float(hf.hs), float(hf.vs), float(hf.ox), float(hf.oy))
    rays = ramp_rays()
    got = s.ray_cast([s.contact_frame(0)], torch.from_numpy(rays).cuda(), align="world", max_range=8.0, normals=True)
    torch.cuda.synchronize()
    t = ramp_analytic(rays)
    n = np.array([-0.25, -0.125, 1.0]) / np.sqrt(0.25 ** 2 + 0.125 ** 2 + 1.0)
    err = float(np.abs(got.dist.cpu().numpy()[0, 0] - t).max()) / 8.0
    print({"ramp": err})
    assert (t > 0.3).all() and (t < 3.0).all()
    assert err <= tolerance("kat_free", "dist")
    assert float(np.abs(got.normals.cpu().numpy()[0, 0] - n).max()) <= tolerance("kat_free", "normals")


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_without_a_heightfield_the_plane_is_hit_at_the_frame_points_height(case):
    """dist is the fp32 -o.z / d.z formed from the frame point refresh_rigid_body_state_tensor gives, to the case's
    tolerance, and the normal is e_z exactly."""
    c = shared(case)
    s = c.s
    saved = c.hf
    try:
        c.set_terrain(None)
        rays = np.array([[0, 0, 0, 0, 0, -1], [0, 0, 0, 0.6, -0.3, -1.0], [0, 0, 0, 0.1, 0.2, 0.5]], np.float32)
        d, nn = c.call(torch.from_numpy(rays).cuda(), "world", max_range=50.0)
        s.refresh_rigid_body_state_tensor()
        torch.cuda.synchronize()
        rb = s.rigid_body_state.view(c.n, s.L, 13).double().cpu().numpy()
        for e in range(c.n):
            for f, (l, off) in enumerate(c.frames):
                pz = np.float32((rb[e, l, :3] + quat_R(rb[e, l, 3:7]) @ np.asarray(off, np.float64))[2])
                want = np.array([-pz / np.float32(-1.0), -pz / np.float32(-1.0), 50.0], np.float32)
                assert float(np.abs(d[e, f] - want).max()) / 50.0 <= tolerance(case, "dist")
                assert np.array_equal(nn[e, f], [[0, 0, 1], [0, 0, 1], [0, 0, 0]])
        assert (d[:, :, :2] > 0.5).all() and (d[:, :, 2] == 50.0).all()
    finally:
        c.set_terrain(saved)


def test_downward_rays_reproduce_the_height_scan():
    """Rays (s, d) = ((a, b, 0), (0, 0, -1)) from the root frame lifted to z = 3: a downward ray's dist is 3 -
    height_scan's surface height at (a, b), to the height scan's own surface tolerance."""
    from tests.height_scan_ref import reference_pattern
    from tests.test_gpu_height_scan import tolerance as scan_tolerance
    c = shared("kat_free")
    s = c.s
    root0 = s.root_state.clone()
    try:
        lifted = c.root.copy()
        lifted[:, 2] = 3.0
        lifted[:, 3:7] = [0.0, 0.0, np.sin(0.4), np.cos(0.4)]      # level, a heading only: the frame point is at z = 3
        s.root_state.copy_(torch.from_numpy(lifted))
        pts = reference_pattern()
        rays = np.zeros((pts.shape[0], 6), np.float32)
        rays[:, :2], rays[:, 5] = pts, -1.0
        frame = [s.contact_frame(0)]
        for align in ("world", "yaw"):
            d, _nn = c.call(torch.from_numpy(rays).cuda(), align, frames=frame)
            h = s.height_scan(frame, torch.from_numpy(pts).cuda(), surface="surface", align=align).heights
            torch.cuda.synchronize()
            h = h.cpu().numpy()
            err = float(np.abs((3.0 - d) - h).max()) / max(float(np.abs(h).max()), 1e-30)
            print({"height_scan": align, "err": err})
            assert (h > 0.05).any() and (h == 0.0).any()
            assert err <= scan_tolerance("kat_free", "h_surface")
    finally:
        s.root_state.copy_(root0)


# ------------------------------------------------------------------ further tests

@pytest.mark.parametrize("case", ["thormang", "kat_free"])
def test_a_non_finite_state_reads_misses_and_leaves_the_other_envs_alone(case):
    """A NaN root position in env 0, an infinite one in env 3 and a NaN joint angle in env 4 (where the case has
    joints; there only the frame the joint carries): every such ray reads max_range exactly with a zero normal, in every alignment, and the rows of
    the other envs keep their bits."""
    c = shared(case)
    s = c.s
    root0, dof0 = s.root_state.clone(), s.dof_state.clone()
    before = {a: c.call("lidar", a) for a in ALIGNS}
    bad = [0, 3] + ([4] if s.D > 0 else [])
    good = [e for e in range(c.n) if e not in bad]
    try:
        s.root_state[0, 1] = float("nan")
        s.root_state[3, 2] = float("inf")
        if s.D > 0:
            s.dof_state.view(c.n, s.D, 2)[4, 0, 0] = float("nan")
        for a in ALIGNS:
            d, nn = c.call("lidar", a)
            if s.D > 0:
                # thormang's first joint (torso_y) carries the head, frame 1 (lidar_link), and neither the pelvis
                # nor the foot: frame 1 must miss, frames 0 and 2 keep their bits
                assert c.case == "thormang" and c.m.joints[0].dof == 0 and c.m.joints[0].parent == 0
                assert (d[4, 1] == np.float32(MAX_RANGE)).all() and not nn[4, 1].any(), a
                assert np.array_equal(d[4, [0, 2]].view(np.uint32), before[a][0][4, [0, 2]].view(np.uint32)), a
            assert (d[[0, 3]] == np.float32(MAX_RANGE)).all() and not nn[[0, 3]].any(), a
            assert np.array_equal(d[good].view(np.uint32), before[a][0][good].view(np.uint32)), a
            assert np.array_equal(nn[good].view(np.uint32), before[a][1][good].view(np.uint32)), a
            assert (before[a][0][[0, 3]] < MAX_RANGE).any()
    finally:
        s.root_state.copy_(root0)
        s.dof_state.copy_(dof0)
    again = c.call("lidar", "link")
    assert all(np.array_equal(x, y) for x, y in zip(again, before["link"]))


def test_an_env_does_not_depend_on_the_other_envs():
    c = shared("thormang")
    s = c.s
    root0, dof0 = s.root_state.clone(), s.dof_state.clone()
    before = {a: c.call("lidar", a) for a in ALIGNS}
    try:
        _m, _f, r2, d2 = scenario("thormang", N, 99)
        r2, d2 = r2.copy(), d2.copy().reshape(c.n, -1, 2)
        r2[1] = c.root[1]                                       # env 1 keeps its state, the others get new ones
        d2[1] = c.dof.reshape(c.n, -1, 2)[1]
        s.root_state.copy_(torch.from_numpy(r2))
        s.dof_state.copy_(torch.from_numpy(np.ascontiguousarray(d2.reshape(-1, 2))))
        for a in ALIGNS:
            d, nn = c.call("lidar", a)
            assert np.array_equal(d[1].view(np.uint32), before[a][0][1].view(np.uint32)), a
            assert np.array_equal(nn[1].view(np.uint32), before[a][1][1].view(np.uint32)), a
            assert not np.array_equal(d[0], before[a][0][0]), a
    finally:
        s.root_state.copy_(root0)
        s.dof_state.copy_(dof0)
    again = c.call("lidar", "link")
    assert all(np.array_equal(x, y) for x, y in zip(again, before["link"]))


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_call_sequence_sees_the_current_heightfield_and_state(case):
    """cast; remove the heightfield; cast; set another heightfield; cast; step; cast; restore; cast -- each against
    the reference on the state read back, and the first bits come back at the end."""
    c = Case(case, seed=73)
    s = c.s

    def state():
        torch.cuda.synchronize()
        return s.root_state.cpu().numpy().copy(), s.dof_state.cpu().numpy().copy()

    def cast_and_check(key):
        root, dof = state()
        got = c.call("lidar", "link")
        c.check(key, got, c.reference("lidar", "link", root=root, dof=dof))
        return got

    first = cast_and_check("first")
    c.set_terrain(None)
    flat = cast_and_check("no heightfield")
    hit = flat[0] < MAX_RANGE
    assert hit.any() and (~hit).any() and (flat[1][hit] == [0, 0, 1]).all()
    c.set_terrain(smooth_heightfield(150, 190, np.random.default_rng(8), vs=0.01, ox=-9.0, oy=-6.5))
    second = cast_and_check("another heightfield")
    assert not np.array_equal(first[0], second[0])
    s.root_state[:, 2] += 0.3                   # clear of the ground: the step is a short free flight
    before = state()
    s.simulate()
    after = state()
    assert not np.array_equal(before[0], after[0])
    third = cast_and_check("after a step")
    assert not np.array_equal(third[0], second[0])
    c.set_terrain(terrain())
    s.root_state.copy_(torch.from_numpy(c.root))
    s.dof_state.copy_(torch.from_numpy(c.dof))
    back = cast_and_check("restored")
    assert np.array_equal(back[0].view(np.uint32), first[0].view(np.uint32))
    assert np.array_equal(back[1].view(np.uint32), first[1].view(np.uint32))


def test_error_paths_launch_nothing():
    from thormang_isaacgym_amd._lib import lib
    c = shared("gogoro")
    s = c.s
    rays = c.rays["lidar"]
    R = rays.shape[0]
    d, nn = _nan(c.n, 1, R), _nan(c.n, 1, R, 3)
    rp = abi.tg_ray_params()
    rp.align, rp.max_range = 0, MAX_RANGE
    fr = (abi.tg_contact_frame * 1)()

    def rejected(frames, F, ry, nr, params, dist, normals, sim=s.handle):
        rc = lib().tg_ray_cast(sim, frames, F, ry, nr, params, dist, normals)
        assert rc == -1 and lib().tg_last_error().startswith(b"tg_ray_cast:"), lib().tg_last_error()

    ok = (fr, 1, rays.data_ptr(), R, rp, d.data_ptr(), nn.data_ptr())
    fr[0].link = s.L                                                      # a link the model does not have
    rejected(*ok)
    fr[0].link = -1
    rejected(*ok)
    fr[0].link = 0
    fr[0].offset[1] = float("inf")
    rejected(*ok)
    fr[0].offset[1] = 0.0
    for k, bad in ((0, None), (1, 0), (1, 9), (2, None), (3, 0), (3, abi.TG_RAY_MAX_RAYS + 1), (4, None)):
        args = list(ok)
        args[k] = bad
        rejected(*args)
    for field, bad in (("align", 3), ("align", -1), ("max_range", 0.0), ("max_range", -1.0),
                       ("max_range", float("inf")), ("max_range", float("nan"))):
        keep = getattr(rp, field)
        setattr(rp, field, bad)
        rejected(*ok)
        setattr(rp, field, keep)
    rejected(fr, 1, rays.data_ptr(), R, rp, None, None)                   # both outputs null
    rejected(*ok, sim=None)                                               # a null sim
    torch.cuda.synchronize()
    assert bool(torch.isnan(d).all()) and bool(torch.isnan(nn).all())     # nothing was launched
    assert lib().tg_ray_cast(s.handle, *ok) == 0                          # (and the accepted call writes everything)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(d).any()) and not bool(torch.isnan(nn).any())


def test_wrapper_checks_and_the_sims_own_tensors():
    c = shared("gogoro")
    s = c.s
    rays = c.rays["lidar"]
    R = rays.shape[0]
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, rays, out=torch.zeros(c.n, 1, R + 1, device="cuda:0"))       # shape
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, rays.double())                                              # dtype
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, rays.cpu())                                                 # device
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, rays[:, :5].contiguous())                                   # not [R, 6]
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, torch.zeros(abi.TG_RAY_MAX_RAYS + 1, 6, device="cuda:0"))    # count
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes * 9, rays)
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, rays, align="roll")
    with pytest.raises(ValueError):
        s.ray_cast(c.cframes, rays, max_range=0.0)
    want = c.call("lidar", "link")
    own = s.ray_cast(c.cframes, rays, align="link", max_range=MAX_RANGE, normals=True)      # the sim's own tensors
    torch.cuda.synchronize()
    assert np.array_equal(own.dist.cpu().numpy(), want[0]) and np.array_equal(own.normals.cpu().numpy(), want[1])
    assert s.ray_cast(c.cframes, rays, max_range=MAX_RANGE).normals is None
    given = _nan(c.n, 1, R)
    assert s.ray_cast(c.cframes, rays, max_range=MAX_RANGE, out=given).dist is given
    az, el = np.deg2rad(3.0 + 22.5 * np.arange(16)), np.deg2rad([-50.0, -30.0, -15.0, -7.0, -2.0, 8.0])
    assert np.allclose(s.lidar_rays(az, el).cpu().numpy(), lidar(), atol=1e-7)
    built = s.pinhole_rays(16, 12, np.deg2rad(87.0))
    assert built.dtype == torch.float32 and tuple(built.shape) == (192, 6)
    assert np.allclose(built.cpu().numpy(), rr.pinhole_pattern(16, 12, np.deg2rad(87.0)), atol=1e-7)


# ------------------------------------------------------------------ the Gogoro task

def _depth_reference(env, hf):
    """The depth image's reference on the state read back."""
    from thormang_isaacgym_amd.tasks.gogoro import Gogoro
    torch.cuda.synchronize()
    root, dof = env.sim.root_state.cpu().numpy(), env.sim.dof_state.cpu().numpy()
    m = env.sim.model
    rays = rr.pinhole_pattern(Gogoro.DEPTH_WIDTH, Gogoro.DEPTH_HEIGHT, Gogoro.DEPTH_HFOV)
    return rr.ray_cast_ref(m, root, dof, [(m.link_index("realsense_link"), (0.0, 0.0, 0.0))], rays, hf, "link",
                           Gogoro.DEPTH_MAX)


def test_gogoro_task_exposes_the_depth_image_on_the_terrain():
    """Gogoro with the Perlin terrain and env.enableDepthCamera: extras["depth"] [N, 24, 32] is the cast of the state
    the step returns with -- the pinhole pattern at realsense_link in the link's axes.  All 16 images of each of the 6
    steps are compared with the reference on the state read back."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from tests.gpu_harness import NumpyDraws, balance_policy, make_gpu_gogoro, parity_cfg
    from thormang_isaacgym_amd.tasks import gogoro as gmod
    n = 16
    torch.manual_seed(5)
    cfg = parity_cfg(n, max_steps=300)
    cfg["env"]["enableDepthCamera"] = True
    saved, gmod.USE_TERAIN = gmod.USE_TERAIN, True
    try:
        env = make_gpu_gogoro(cfg, NumpyDraws(0))
    finally:
        gmod.USE_TERAIN = saved
    t = env.terrain
    o = -float(env._terrain_start_mid)
    hf = Heightfield(t.heightsamples.cpu().numpy().astype(np.float32), np.float32(t.V_scale), np.float32(t.H_scale),
                     np.float32(o), np.float32(o))
    assert np.allclose(env.depth_rays.cpu().numpy(), rr.pinhole_pattern(32, 24, np.deg2rad(87.0)), atol=1e-7)
    bound = gmod.Gogoro.DEPTH_MAX
    obs = np.zeros((n, 6), np.float32)
    worst, hits, terrain_hits = 0.0, 0, 0
    for k in range(6):
        act = torch.from_numpy(balance_policy(obs)).cuda()
        od, _rew, _reset, extras = env.step(act)
        obs = od["obs"].cpu().numpy()
        depth = extras["depth"]
        assert tuple(depth.shape) == (n, 24, 32) and depth.dtype == torch.float32
        got = depth.cpu().numpy().reshape(n, -1)
        assert not np.isnan(got).any() and (got <= bound).all() and (got >= 0).all()
        ref = _depth_reference(env, hf)                    # every env, every step
        keep = rr.keep_dist(ref)[:, 0]
        assert 1.0 - keep.mean() <= rr.EXCLUDED_CAP
        assert np.array_equal((got < bound)[keep], (ref.dist[:, 0] < bound)[keep])
        worst = max(worst, float(np.abs(got - ref.dist[:, 0])[keep].max()) / bound)
        hits += int((got < bound).sum())
        terrain_hits += int((ref.kind == rr.TRIANGLE).sum())
    print({"case": "gogoro_task", "dist": worst, "hits": hits, "terrain_hits": terrain_hits})
    assert hits > 100 and terrain_hits > 0
    assert worst <= tolerance("gogoro_task", "dist")


def test_gogoro_task_is_unchanged_by_the_switch_and_sees_the_plane_on_flat_ground():
    """16 envs, 20 steps, env.enableDepthCamera on against off on the flat ground: obs, reward, reset and the sim state
    bit-identical; the key is absent with the switch off; every pixel is the analytic plane depth or the bound."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from tests.gpu_harness import NumpyDraws, balance_policy, make_gpu_gogoro, parity_cfg
    from thormang_isaacgym_amd.tasks.gogoro import Gogoro
    n = 16
    envs = []
    for on in (False, True):
        cfg = parity_cfg(n, max_steps=300)
        if on:
            cfg["env"]["enableDepthCamera"] = True
        envs.append(make_gpu_gogoro(cfg, NumpyDraws(3)))
    off, on = envs
    assert off.depth is None and "depth" not in off.extras
    obs = np.zeros((n, 6), np.float32)
    worst = 0.0
    for k in range(20):
        act = torch.from_numpy(balance_policy(obs)).cuda()
        o0, r0, z0, x0 = off.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        assert torch.equal(o0["obs"], o1["obs"]) and torch.equal(r0, r1) and torch.equal(z0, z1)
        assert torch.equal(x0["time_outs"], x1["time_outs"]) and "depth" not in x0
        depth = x1["depth"]
        assert tuple(depth.shape) == (n, 24, 32)
        ref = _depth_reference(on, None)                     # the plane alone: -o.z / d.z or the bound
        keep = rr.keep_dist(ref)[:, 0]
        got = depth.cpu().numpy().reshape(n, -1)
        assert np.array_equal((got < Gogoro.DEPTH_MAX)[keep], (ref.dist[:, 0] < Gogoro.DEPTH_MAX)[keep])
        assert (got[got >= Gogoro.DEPTH_MAX] == Gogoro.DEPTH_MAX).all()
        worst = max(worst, float(np.abs(got - ref.dist[:, 0])[keep].max()) / Gogoro.DEPTH_MAX)
        assert (ref.kind[ref.dist < Gogoro.DEPTH_MAX] == rr.PLANE).all() and (got < Gogoro.DEPTH_MAX).any()
        obs = o0["obs"].cpu().numpy()
    print({"case": "gogoro_task", "flat": worst})
    assert worst <= tolerance("gogoro_task", "dist")
    assert torch.equal(off.sim.root_state, on.sim.root_state) and torch.equal(off.sim.dof_state, on.sim.dof_state)
