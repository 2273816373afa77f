"""The height scan on the GPU (tg_height_scan, Sim.height_scan) against the
float64 reference (tests/height_scan_ref.py, pinned by
tests/test_height_scan_reference.py).

Sims of five envs and of one.  States from random_state; a root quaternion is
redrawn until w^2 + z^2 >= 0.1 for every scanned link (below that the heading is
ill-conditioned); env 1 stands at (40.07, 30.11), tens of metres from env 0 and still
on the grid, env 2 at the grid's edge so that part of its pattern falls off it.
The heightfield is 200 x 168 samples, hs = 0.25, vs = 0.005, origin (-7, -4.5):
smooth, a few decimetres high, with negative patches.  Patterns: the
reference's 140 points (F P = 420 with three frames: more than 64 and no
multiple of it) and a single point.  Every output is filled with NaN before
each call.

Exclusion.  A sample nearer than MARGIN_CELLS = 1e-3 cells to a discontinuity
of the output compared (height_scan_ref's margins) is left out: 2.5e-4 m, and
asserted below to be at least 8 fp32 ulps of the largest coordinate the envs
stand at.  At most 2 % of a case may be left out (asserted here and, from the
reference alone, in tests/test_height_scan_reference.py).

Tolerance.  max |got - ref| / max |ref| (normals: scale 1) was measured per
case and output on the MI355X on this file's first run (SCAN_MEASURED below;
the worst over every comparison the file makes for the case).  Asserted: 4 x
the measured value, under the project's hard cap of 1e-4.  Worst measured:
surface heights 3.4e-6 (thormang), cell heights 4.6e-8, normals 5.9e-8, the
relative map 7.7e-7; at most 0.95 % of a comparison's samples were left out.
The exact checks take no tolerance."""
import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.height_scan_ref import (EXCLUDED_CAP, MARGIN_CELLS, Heightfield, height_scan_ref, reference_pattern,
                                   smooth_heightfield)
from tests.jacobian_ref import quat_R
from tests.oracle_lib import rigid_body_states
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

N = 5
FAR = (40.07, 30.11)        # env 1 (off the grid's lattice: a world-aligned pattern must not sit on cell lines)
EDGE = (-6.63, 12.04)       # env 2: x within a pattern's reach of the grid's edge at -7
CASES = ["thormang", "gogoro", "jit_walker", "kat_free"]
ALIGNS = ["yaw", "world", "link"]
OUTPUTS = ["h_surface", "h_cell", "normals", "relative"]
RELATIVE = dict(bias=0.5, lo=-1.0, hi=1.0, scale=5.0)     # line 302 of the reference with heightMeasurementScale 5
# max |got - ref| / max |ref| per output, measured on the MI355X: the worst over every comparison this file makes
# for the case (alignments, the five-env, one-env and single-point sims, the call sequence's other terrain and
# stepped state, the relative map without terrain).  The surface heights carry the fp32 rounding of a coordinate of
# 40 m times the slope; the cell rule picks a sample and the normals a triangle, so they are good to an fp32 ulp
SCAN_MEASURED = {
    #              h_surface h_cell  normals relative
    "thormang":    [3.4e-6, 4.6e-8, 5.9e-8, 7.7e-7],
    "gogoro":      [2.3e-6, 4.5e-8, 5.4e-8, 5.3e-7],
    "jit_walker":  [2.0e-6, 4.6e-8, 5.6e-8, 5.5e-7],
    "kat_free":    [3.1e-6, 4.5e-8, 5.4e-8, 7.4e-7],
    "gogoro_task": [1.2e-6, None, None, None],          # (the task test compares the surface heights only)
}
HARD_CAP = 1e-4
assert all(4 * v <= HARD_CAP for row in SCAN_MEASURED.values() for v in row if v is not None)


def tolerance(case, output):
    return 4 * dict(zip(OUTPUTS, SCAN_MEASURED[case]))[output]


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return {"jit_walker": pm.jit_walker, "kat_free": pm.free_body}.get(name, lambda: load_model(name))()


def case_frames(case, m):
    """(link index, offset) pairs of a case."""
    if case == "thormang":
        from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
        lf, rf = walk_feet_indices(m)
        return [(0, (0.0, 0.0, 0.0)), (lf, (0.05, 0.01, -0.03)), (rf, (-0.02, 0.03, -0.03))]
    if case == "gogoro":
        return [(0, (0.0, 0.0, 0.0))]
    if case == "jit_walker":
        return [(0, (0.0, 0.0, 0.0)), (m.num_bodies - 1, (0.1, 0.0, -0.05))]
    return [(0, (0.2, -0.1, 0.05)), (0, (0.0, 0.0, 0.0))]        # kat_free: one link in two frames


def terrain(seed=7):
    return smooth_heightfield(200, 168, np.random.default_rng(seed))


def scenario(case, n=N, seed=61):
    """(model, frames, root, dof) of a case: no GPU needed (the reference test reads it too)."""
    m = _model(case)
    frames = case_frames(case, m)
    rs = np.random.default_rng(seed)
    root, dof = random_state(m, n, rs)
    if n > 1:
        root[1, :2] = FAR
        root[2, :2] = EDGE
    desc = abi.ModelDesc(m)
    for e in range(n):
        for _ in range(1000):
            q = rigid_body_states(desc, root[e:e + 1], dof[e * m.num_dof:(e + 1) * m.num_dof])[0, :, 3:7]
            q = q.astype(np.float64) / np.linalg.norm(q, axis=1, keepdims=True)
            if all(q[l, 3] ** 2 + q[l, 2] ** 2 >= 0.1 for l, _o in frames):
                break
            v = rs.normal(0, 1, 4)
            root[e, 3:7] = v / np.linalg.norm(v)
        else:
            raise AssertionError("no well-conditioned heading found")
    return m, frames, root, dof


def modes():
    """(key, surface, align, normals, relative, output compared) of every call a case makes."""
    out = []
    for al in ALIGNS:
        out.append((f"surface/{al}", "surface", al, True, None, "h_surface"))
        out.append((f"cell/{al}", "cell", al, False, None, "h_cell"))
        out.append((f"surface/{al}/relative", "surface", al, False, RELATIVE, "relative"))
    out.append(("cell/yaw/relative", "cell", "yaw", False, RELATIVE, "relative"))
    return out


def excluded_share(margin):
    return float((margin < MARGIN_CELLS).mean())


def test_margin_covers_the_rounding_of_the_env_placement():
    hf = terrain()
    reach = max(abs(FAR[0]), abs(FAR[1]), abs(EDGE[0]), abs(EDGE[1])) + 3.0      # the robots' and the patterns' reach
    assert MARGIN_CELLS * float(hf.hs) >= 8 * float(np.spacing(np.float32(reach)))
    assert hf.heights.shape[0] != hf.heights.shape[1] and float(hf.vs) != 1.0 and float(hf.hs) == 0.25
    assert float(hf.ox) != float(hf.oy) and float(hf.ox) != 0.0 and float(hf.oy) != 0.0
    z = float(hf.vs) * hf.heights
    assert z.min() < -0.1 and 0.2 < z.max() < 0.5
    # both far envs stand on the grid
    for x, y in (FAR, EDGE):
        u, v = (x - float(hf.ox)) / float(hf.hs), (y - float(hf.oy)) / float(hf.hs)
        assert 0 < u < hf.heights.shape[0] - 1 and 0 < v < hf.heights.shape[1] - 1


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")


class Case:
    """A sim of ``n`` envs in the test state on the test terrain, with every mode's call made and its reference."""

    def __init__(self, case, n=N, seed=61, points=None):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.case, self.n = case, n
        self.m, self.frames, self.root, self.dof = scenario(case, n, seed)
        m = self.m
        self.hf = terrain()
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        s.refresh()
        self.set_terrain(self.hf)
        self.pts_np = reference_pattern() if points is None else np.asarray(points, np.float32)
        self.pts = torch.from_numpy(self.pts_np).cuda()
        self.F, self.P = len(self.frames), self.pts_np.shape[0]
        self.cframes = [s.contact_frame(l, o) for l, o in self.frames]
        self.got, self.ref = {}, {}
        for key, surface, align, normals, relative, _o in modes():
            self.got[key] = self.call(surface, align, normals, relative)
            self.ref[key] = self.reference(surface, align, relative)

    def set_terrain(self, hf):
        self.hf = hf
        if hf is None:
            self.s.set_heightfield(None)
        else:
            self.s.set_heightfield(hf.heights, float(hf.hs), float(hf.vs), float(hf.ox), float(hf.oy))

    def call(self, surface, align, normals=False, relative=None):
        """One call on NaN-filled outputs; (heights, normals) as numpy, normals all NaN when not asked for."""
        h, nn = _nan(self.n, self.F, self.P), _nan(self.n, self.F, self.P, 3)
        got = self.s.height_scan(self.cframes, self.pts, surface=surface, align=align, normals=normals,
                                 relative=relative, out=h, out_normals=nn if normals else None)
        assert got.heights is h and got.normals is (nn if normals else None)
        torch.cuda.synchronize()
        return h.cpu().numpy(), nn.cpu().numpy()

    def reference(self, surface, align, relative=None, root=None, dof=None):
        return height_scan_ref(self.m, self.root if root is None else root, self.dof if dof is None else dof,
                               self.frames, self.pts_np, self.hf, surface, align, relative)

    def figures(self, key, output, got=None, ref=None):
        """max |got - ref| / max |ref| of the compared output over the samples kept, and the share left out;
        asserts that every element was written."""
        h, nn = self.got[key] if got is None else got
        ref = self.ref[key] if ref is None else ref
        assert h.dtype == np.float32 and not np.isnan(h).any()
        keep = ref.margin >= MARGIN_CELLS
        fig = {output: float(np.abs(h - ref.heights)[keep].max()) / max(float(np.abs(ref.heights).max()), 1e-30),
               "excluded": excluded_share(ref.margin)}
        if ref.normals is not None and not np.isnan(nn).all():
            assert not np.isnan(nn).any()
            keep_n = ref.margin_normals >= MARGIN_CELLS
            fig["normals"] = float(np.abs(nn - ref.normals)[keep_n].max())
            fig["excluded_normals"] = excluded_share(ref.margin_normals)
            assert float(np.abs(np.linalg.norm(nn, axis=-1) - 1.0).max()) <= 1e-6
        return fig

    def check(self, key, output, got=None, ref=None):
        fig = self.figures(key, output, got, ref)
        print({"case": self.case, "n": self.n, "P": self.P, "mode": key, **fig})
        assert fig["excluded"] <= EXCLUDED_CAP and fig.get("excluded_normals", 0.0) <= EXCLUDED_CAP, fig
        assert fig[output] <= tolerance(self.case, output), (key, fig)
        if "normals" in fig:
            assert fig["normals"] <= tolerance(self.case, "normals"), (key, fig)
        return fig


_cases = {}


def shared(case):
    if case not in _cases:
        _cases[case] = Case(case)
    return _cases[case]


@pytest.mark.parametrize("case", CASES)
def test_outputs_match_the_reference(case):
    c = shared(case)
    worst = {}
    for key, _s, _a, _n, _r, output in modes():
        for k, v in c.check(key, output).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print({"case": case, "worst": worst})
    # the scan saw terrain, plane and off-grid samples, and the clamp of the relative map bit on both sides
    r = c.ref["surface/yaw"]
    assert (r.heights > 0.05).any() and (r.heights == 0.0).any() and np.isinf(r.margin).sum() == 0
    off = ~np.isfinite(r.margin_normals) | (r.normals[..., 2] == 1.0)
    assert off.any() and (r.normals[..., 2] < 0.999).any()
    rel = c.ref["surface/yaw/relative"].heights
    assert (rel == 5.0).any() or (rel == -5.0).any()
    assert ((rel > -5.0) & (rel < 5.0)).any()


@pytest.mark.parametrize("case", ["thormang", "gogoro", "kat_free"])
def test_one_env(case):
    c = Case(case, n=1, seed=62)
    for key, _s, _a, _n, _r, output in modes():
        c.check(key, output)


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_single_point_pattern(case):
    c = Case(case, points=[[0.3, -0.2]])
    assert c.P == 1
    for key, _s, _a, _n, _r, output in modes():
        c.check(key, output)


def test_runtime_loaded_model():
    """jit_walker is compiled at run time (tg_model_jit): the call works, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = shared("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_frame_points_agree_with_the_rigid_body_state_tensor_and_relative_without_terrain(case):
    """Without a heightfield the relative heights are the clamp of p_f.z - bias, p_f from
    refresh_rigid_body_state_tensor; heights are 0.0 and normals e_z exactly."""
    c = shared(case)
    s = c.s
    saved = c.hf
    try:
        c.set_terrain(None)
        rel = dict(bias=0.25, lo=-0.6, hi=0.9, scale=2.0)
        h, _nn = c.call("surface", "yaw", relative=rel)
        hc, _nn = c.call("cell", "link", relative=rel)
        s.refresh_rigid_body_state_tensor()
        torch.cuda.synchronize()
        rb = s.rigid_body_state.view(c.n, s.L, 13).double().cpu().numpy()
        pz = np.zeros((c.n, c.F))
        for e in range(c.n):
            for f, (l, off) in enumerate(c.frames):
                pz[e, f] = (rb[e, l, :3] + quat_R(rb[e, l, 3:7]) @ np.asarray(off, np.float64))[2]
        want = np.clip(pz - rel["bias"], rel["lo"], rel["hi"]) * rel["scale"]
        want = np.broadcast_to(want[:, :, None], h.shape)
        scale = float(np.abs(want).max())
        d = max(float(np.abs(h - want).max()), float(np.abs(hc - want).max())) / scale
        print({"case": case, "relative_without_terrain": d})
        assert d <= tolerance(case, "relative")
        assert (np.abs(want) < rel["scale"] * 0.59).any()                       # (not everything sits on the clamp)
        for surface, align, normals in (("surface", "yaw", True), ("surface", "world", True),
                                        ("surface", "link", True), ("cell", "yaw", False)):
            h0, n0 = c.call(surface, align, normals)
            assert np.array_equal(h0.view(np.uint32), np.zeros_like(h0).view(np.uint32))
            if normals:
                ez = np.zeros_like(n0)
                ez[..., 2] = 1.0
                assert np.array_equal(n0.view(np.uint32), ez.view(np.uint32))
    finally:
        c.set_terrain(saved)
    again = c.call("surface", "yaw", True)
    assert all(np.array_equal(x, y) for x, y in zip(again, c.got["surface/yaw"]))


class Exact:
    """gogoro, identity root poses at power-of-two coordinates, the pattern a lattice of the grid's pitch."""

    def __init__(self):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.m = m = _model("gogoro")
        self.n = n = 3
        self.hf = hf = terrain()
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
        root = np.zeros((n, 13), np.float32)
        root[:, 6] = 1.0
        root[:, :3] = [[2.0, 1.5, 1.0], [32.0, 16.0, 0.5], [-4.0, 8.0, 2.0]]
        s.root_state.copy_(torch.from_numpy(root))
        s.dof_state.zero_()
        s.refresh()
        s.set_heightfield(hf.heights, float(hf.hs), float(hf.vs), float(hf.ox), float(hf.oy))
        self.root = root
        k = np.arange(-6, 7, dtype=np.float32) * np.float32(0.25)
        gx, gy = np.meshgrid(k, k[:9], indexing="ij")
        self.lattice = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)
        self.frame = [s.contact_frame(0)]

    def scan(self, pts, surface):
        p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
        h = _nan(self.n, 1, p.shape[0])
        self.s.height_scan(self.frame, p, surface=surface, align="world", out=h)
        torch.cuda.synchronize()
        return h.cpu().numpy()[:, 0]

    def indices(self, pts):
        """The integer grid coordinates (i, j) [N, P] of root + pts, exact in float32."""
        hf = self.hf
        x = self.root[:, None, 0] + pts[None, :, 0]
        y = self.root[:, None, 1] + pts[None, :, 1]
        u, v = (x - hf.ox) / hf.hs, (y - hf.oy) / hf.hs
        return u, v


def test_vertices_and_cell_centres_are_exact():
    """SURFACE at interior vertices is vs hf[i][j] bit for bit where that is positive (0.0 elsewhere): a row/column
    transposition cannot pass on a non-square field.  CELL at cell centres is vs min(hf[i][j], hf[i+1][j+1])."""
    x = Exact()
    hf = x.hf
    H, vs = hf.heights, np.float32(hf.vs)
    rows, cols = H.shape
    u, v = x.indices(x.lattice)
    assert np.array_equal(u, np.rint(u)) and np.array_equal(v, np.rint(v))
    i, j = u.astype(int), v.astype(int)
    assert i.min() >= 1 and i.max() <= rows - 2 and j.min() >= 1 and j.max() <= cols - 2      # interior
    got = x.scan(x.lattice, "surface")
    raw = (vs * H[i, j]).astype(np.float32)
    want = np.where(raw > 0, raw, np.float32(0.0)).astype(np.float32)
    assert (raw > 0).sum() > 50 and (raw <= 0).sum() > 5
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    centres = x.lattice + np.float32(0.125)
    u, v = x.indices(centres)
    i, j = np.floor(u).astype(int), np.floor(v).astype(int)
    assert np.array_equal(u - i, np.full_like(u, 0.5)) and np.array_equal(v - j, np.full_like(v, 0.5))
    got = x.scan(centres, "cell")
    want = (vs * np.minimum(H[i, j], H[i + 1, j + 1])).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want < 0).any() and (want > 0).any()


def test_an_env_does_not_depend_on_the_other_envs():
    c = shared("thormang")
    s = c.s
    root0, dof0 = s.root_state.clone(), s.dof_state.clone()
    try:
        r2, d2 = random_state(c.m, c.n, np.random.default_rng(77))
        d2 = d2.reshape(c.n, -1, 2)
        r2[1] = c.root[1]                                       # env 1 keeps its state, the others get new ones
        d2[1] = c.dof.reshape(c.n, -1, 2)[1]
        s.root_state.copy_(torch.from_numpy(r2))
        s.dof_state.copy_(torch.from_numpy(np.ascontiguousarray(d2.reshape(-1, 2))))
        for key, surface, align, normals, relative, _o in modes():
            h, nn = c.call(surface, align, normals, relative)
            h0, n0 = c.got[key]
            assert np.array_equal(h[1].view(np.uint32), h0[1].view(np.uint32)), key
            assert np.array_equal(nn[1].view(np.uint32), n0[1].view(np.uint32)), key
            assert not np.array_equal(h[0], h0[0]), key
    finally:
        s.root_state.copy_(root0)
        s.dof_state.copy_(dof0)
    again = c.call("surface", "yaw", True)
    assert all(np.array_equal(x, y) for x, y in zip(again, c.got["surface/yaw"]))


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_call_sequence_sees_the_current_heightfield_and_state(case):
    """scan; remove the heightfield; scan (zeros); set another heightfield; scan; step; scan -- each against the
    reference on the state read back."""
    c = Case(case, seed=63)
    s = c.s

    def state():
        torch.cuda.synchronize()
        return s.root_state.cpu().numpy().copy(), s.dof_state.cpu().numpy().copy()

    def scan_and_check():
        root, dof = state()
        got = c.call("surface", "yaw", True)
        c.check("surface/yaw", "h_surface", got, c.reference("surface", "yaw", root=root, dof=dof))
        gotc = c.call("cell", "yaw")
        c.check("cell/yaw", "h_cell", gotc, c.reference("cell", "yaw", root=root, dof=dof))
        return got, gotc

    first, firstc = scan_and_check()
    c.set_terrain(None)
    h, nn = c.call("surface", "yaw", True)
    assert not h.any() and not nn[..., :2].any() and (nn[..., 2] == 1.0).all()
    assert not c.call("cell", "yaw")[0].any()
    other = smooth_heightfield(150, 190, np.random.default_rng(8), vs=0.01, ox=-9.0, oy=-6.5)
    c.set_terrain(other)
    second, _ = scan_and_check()
    assert not np.array_equal(first[0], second[0])
    # lift the robots clear of the ground so that the step is a short free flight, then step
    s.root_state[:, 2] += 3.0
    s.root_state[:, 7:13] *= 0.1
    before = state()
    s.simulate()
    after = state()
    assert not np.array_equal(before[0], after[0])
    third, _ = scan_and_check()
    assert not np.array_equal(third[0], second[0])
    c.set_terrain(terrain())
    s.root_state.copy_(torch.from_numpy(c.root))
    s.dof_state.copy_(torch.from_numpy(c.dof))
    back, backc = scan_and_check()
    assert np.array_equal(back[0], first[0]) and np.array_equal(back[1], first[1])
    assert np.array_equal(backc[0], firstc[0])


def test_gogoro_task_exposes_measured_heights_on_the_terrain():
    """Gogoro with the Perlin terrain and env.enableHeightScan: extras["measured_heights"] [N, 140] is the scan of
    the state the step returns with -- the reference pattern about the root link, yaw aligned, the surface rule."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from tests.gpu_harness import NumpyDraws, balance_policy, make_gpu_gogoro, parity_cfg
    from thormang_isaacgym_amd.tasks import gogoro as gmod
    n = 16
    torch.manual_seed(5)
    cfg = parity_cfg(n, max_steps=300)
    cfg["env"]["enableHeightScan"] = True
    saved, gmod.USE_TERAIN = gmod.USE_TERAIN, True
    try:
        env = make_gpu_gogoro(cfg, NumpyDraws(0))
    finally:
        gmod.USE_TERAIN = saved
    t = env.terrain
    o = -float(env._terrain_start_mid)
    hf = Heightfield(t.heightsamples.cpu().numpy().astype(np.float32), np.float32(t.V_scale), np.float32(t.H_scale),
                     np.float32(o), np.float32(o))
    assert np.array_equal(env.height_points.cpu().numpy(), reference_pattern())
    obs = np.zeros((n, 6), np.float32)
    worst, seen = 0.0, 0.0
    for k in range(6):
        act = torch.from_numpy(balance_policy(obs)).cuda()
        od, _rew, _reset, extras = env.step(act)
        obs = od["obs"].cpu().numpy()
        mh = extras["measured_heights"]
        assert tuple(mh.shape) == (n, 140) and mh.dtype == torch.float32
        torch.cuda.synchronize()
        root, dof = env.sim.root_state.cpu().numpy(), env.sim.dof_state.cpu().numpy()
        ref = height_scan_ref(env.sim.model, root, dof, [(0, (0.0, 0.0, 0.0))], reference_pattern(), hf, "surface",
                              "yaw")
        keep = ref.margin[:, 0] >= MARGIN_CELLS
        assert excluded_share(ref.margin) <= EXCLUDED_CAP
        got = mh.cpu().numpy()
        assert not np.isnan(got).any()
        d = float(np.abs(got - ref.heights[:, 0])[keep].max()) / float(np.abs(ref.heights).max())
        worst, seen = max(worst, d), max(seen, float(np.abs(ref.heights).max()))
    print({"case": "gogoro_task", "h_surface": worst, "max_height": seen})
    assert seen > 0.01
    assert worst <= tolerance("gogoro_task", "h_surface")


def test_gogoro_task_is_unchanged_by_the_switch_and_reads_zeros_on_flat_ground():
    """16 envs, 20 steps, env.enableHeightScan on against off on the flat ground: obs, reward and reset bit-identical;
    the key is absent with the switch off; the heights are zeros."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from tests.gpu_harness import NumpyDraws, balance_policy, make_gpu_gogoro, parity_cfg
    n = 16
    envs = []
    for on in (False, True):
        cfg = parity_cfg(n, max_steps=300)
        if on:
            cfg["env"]["enableHeightScan"] = True
        envs.append(make_gpu_gogoro(cfg, NumpyDraws(3)))
    off, on = envs
    assert off.measured_heights is None and "measured_heights" not in off.extras
    obs = np.zeros((n, 6), np.float32)
    for _ in range(20):
        act = torch.from_numpy(balance_policy(obs)).cuda()
        o0, r0, z0, x0 = off.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        assert torch.equal(o0["obs"], o1["obs"]) and torch.equal(r0, r1) and torch.equal(z0, z1)
        assert torch.equal(x0["time_outs"], x1["time_outs"]) and "measured_heights" not in x0
        mh = x1["measured_heights"]
        assert tuple(mh.shape) == (n, 140) and not bool(mh.any())
        obs = o0["obs"].cpu().numpy()
    assert torch.equal(off.sim.root_state, on.sim.root_state) and torch.equal(off.sim.dof_state, on.sim.dof_state)


def test_error_paths_launch_nothing():
    from thormang_isaacgym_amd._lib import lib
    c = shared("gogoro")
    s = c.s
    h, nn = _nan(c.n, 1, c.P), _nan(c.n, 1, c.P, 3)
    sp = abi.tg_scan_params()
    fr = (abi.tg_contact_frame * 1)()

    def rejected(frames, F, pts, P, params, heights, normals):
        rc = lib().tg_height_scan(s.handle, frames, F, pts, P, params, heights, normals)
        assert rc == -1 and lib().tg_last_error().startswith(b"tg_height_scan:"), lib().tg_last_error()

    ok = (fr, 1, c.pts.data_ptr(), c.P, sp, h.data_ptr(), nn.data_ptr())
    fr[0].link = s.L                                                      # a link the model does not have
    rejected(*ok)
    fr[0].link = 0
    for k, bad in ((0, None), (1, 0), (1, 9), (2, None), (3, 0), (3, 1025), (4, None)):
        args = list(ok)
        args[k] = bad
        rejected(*args)
    for field, bad in (("surface", 2), ("align", 3)):
        setattr(sp, field, bad)
        rejected(*ok)
        setattr(sp, field, 0)
    sp.relative, sp.bias, sp.scale, sp.lo, sp.hi = 1, float("nan"), 1.0, 0.0, 1.0
    rejected(*ok)
    sp.bias, sp.lo = 0.0, 2.0
    rejected(*ok)
    sp.relative, sp.surface = 0, abi.TG_SCAN_CELL
    rejected(*ok)                                                         # normals with the cell rule
    sp.surface = 0
    rejected(fr, 1, c.pts.data_ptr(), c.P, sp, None, None)
    assert lib().tg_height_scan(None, fr, 1, c.pts.data_ptr(), c.P, sp, h.data_ptr(), None) == -1      # a null sim
    torch.cuda.synchronize()
    assert bool(torch.isnan(h).all()) and bool(torch.isnan(nn).all())     # nothing was launched
    with pytest.raises(ValueError):
        s.height_scan(c.cframes, c.pts, out=torch.zeros(c.n, 1, c.P + 1, device="cuda:0"))      # shape
    with pytest.raises(ValueError):
        s.height_scan(c.cframes, c.pts.double())                                              # dtype
    with pytest.raises(ValueError):
        s.height_scan(c.cframes, c.pts.cpu())                                                 # device
    with pytest.raises(ValueError):
        s.height_scan(c.cframes, c.pts, surface="cell", normals=True)
    with pytest.raises(ValueError):
        s.height_scan(c.cframes, c.pts, align="roll")
    with pytest.raises(ValueError):
        s.height_scan(c.cframes * 9, c.pts)
    with pytest.raises(ValueError):
        s.height_scan(c.cframes, c.pts, relative=dict(bias=0.5))
    own = s.height_scan(c.cframes, c.pts, normals=True)                                       # the sim's own tensors
    torch.cuda.synchronize()
    assert np.array_equal(own.heights.cpu().numpy(), c.got["surface/yaw"][0])
    assert np.array_equal(own.normals.cpu().numpy(), c.got["surface/yaw"][1])
    assert s.height_scan(c.cframes, c.pts).normals is None
    grid = s.scan_grid(0.1 * torch.tensor([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8], dtype=torch.float32),
                       0.1 * torch.tensor([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], dtype=torch.float32))
    assert np.array_equal(grid.cpu().numpy(), reference_pattern())
