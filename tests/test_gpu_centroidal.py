"""Centroidal quantities on the GPU (tg_centroidal, Sim.centroidal) against the
float64 reference built from the oracle (tests/centroidal_ref.py, pinned by
tests/test_centroidal_reference.py).

Five envs (no multiple of anything) and a case of one, env 1 far out on the
grid at (300, -200, 1), random root pose, random root and joint velocities,
every sim with a body mass scale U(0.8, 1.2) per link, every output filled
with NaN before each call.

Tolerance.  Per output block -- the com relative to the root position, the com
velocity, the angular momentum, the mass, the centroidal inertia, the linear
and the angular rows of A, the linear and the angular rows of the bias --
max |got - ref| / max |ref| was measured on the MI355X on this file's first
run (CENTROIDAL_MEASURED below, per case and block; a block whose reference is
identically zero, which only the single body has, is judged on the scale of
its whole output; the com block counts what is left of |c - c_ref| beyond one
fp32 ulp of the absolute coordinate).  Asserted: 4 x the worst measured value of the case, under
the project's hard cap of 1e-4 relative.  state[0:3] itself is compared as
|c - c_ref| <= tol max |c_ref - root_pos| + 1 fp32 ulp of |c_ref|: at
(300, -200, 1) an fp32 coordinate cannot do better.  The far env is held to the
same bounds.  The identities against the GPU's own mass-matrix and
inverse-dynamics tensors take the same bound on the same scale.  Measured
worst block per case: thormang 7.0e-7 (the angular bias), gogoro 4.9e-7,
jit_walker 8.5e-7 (k), the single body 3.5e-7, thormang with a fixed base
9.0e-7 (k); the identities 2.2e-7 at most."""
import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.centroidal_ref import bias_ref, com_relative, matrix_ref, state_ref
from tests.id_ref import Kinematics, generalised_velocity
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

FAR = (300.0, -200.0, 1.0)
N = 5
CASES = ["thormang", "gogoro", "jit_walker", "kat_free", "thormang_fix_base"]
BLOCKS = ["c_rel", "cdot", "k", "M", "IG", "A_lin", "A_ang", "bias_lin", "bias_ang"]
# max |got - ref| / max |ref| per block, the worst of the case's five-env and one-env sims, measured on the MI355X
CENTROIDAL_MEASURED = {
    #                     c_rel    cdot     k        M        IG       A_lin    A_ang    bias_lin bias_ang
    "thormang":          [1.9e-7, 2.6e-7, 3.8e-7, 1.6e-7, 3.8e-7, 1.6e-7, 3.5e-7, 4.2e-7, 7.0e-7],
    "gogoro":            [1.6e-7, 1.8e-7, 1.8e-7, 1.5e-7, 4.9e-7, 1.5e-7, 4.3e-7, 2.0e-7, 2.7e-7],
    "jit_walker":        [8.8e-8, 1.2e-7, 8.5e-7, 5.2e-8, 3.9e-7, 5.2e-8, 3.8e-7, 3.8e-7, 7.6e-7],
    "kat_free":          [0.0,    7.9e-8, 1.5e-7, 0.0,    3.1e-7, 0.0,    3.1e-7, 0.0,    3.5e-7],
    "thormang_fix_base": [1.9e-7, 7.5e-7, 9.0e-7, 1.6e-7, 3.8e-7, 1.6e-7, 3.5e-7, 3.9e-7, 3.4e-7],
}
CENTROIDAL_MEASURED = {k: dict(zip(BLOCKS, v)) for k, v in CENTROIDAL_MEASURED.items()}
assert all(4 * max(v.values()) <= 1e-4 for v in CENTROIDAL_MEASURED.values())
FORMS = {"state": (False, False), "matrix": (True, False), "bias": (False, True), "all": (True, True)}


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return {"jit_walker": pm.jit_walker, "kat_free": pm.free_body}.get(name, lambda: load_model(name))()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")


class Case:
    """A sim of ``n`` envs in the test state with the reference's inputs and the reference itself."""

    def __init__(self, case, n=N, seed=41):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        fix_base = case.endswith("_fix_base")
        self.case, self.m, self.n = case, _model(case.replace("_fix_base", "")), n
        m = self.m
        self.D, self.L = D, L = m.num_dof, m.num_bodies
        rs = np.random.default_rng(seed)
        self.root, self.dof = random_state(m, n, rs)
        if n > 1:
            self.root[1, :3] = FAR
        if fix_base:
            self.root[:, 7:13] = 0.0
        self.ms = rs.uniform(0.8, 1.2, (n, L)).astype(np.float32)
        ao = dict(fix_base_link=True) if fix_base else {}
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1, **ao)[1], n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        s.set_body_mass_scale_indexed(torch.from_numpy(self.ms).cuda(), torch.arange(n, device="cuda:0"))
        s.refresh()
        self.kin = Kinematics(m, self.root, self.dof)
        self.u = generalised_velocity(m, self.root, self.dof)
        self.ref_state = state_ref(m, self.root, self.dof, self.ms, self.kin.desc)
        self.ref_A = matrix_ref(m, self.root, self.dof, self.ms, self.kin)
        self.ref_bias = bias_ref(m, self.root, self.dof, self.ms, self.kin)
        _M, self.c_rel = com_relative(self.kin, self.ms)
        self.tol = 4 * max(CENTROIDAL_MEASURED[case].values())

    def call(self, matrix=False, bias=False):
        """One call on NaN-filled outputs, all three buffers handed over whether the call asks for them or not."""
        st, mt, bt = _nan(self.n, 16), _nan(self.n, 6, 6 + self.D), _nan(self.n, 6)
        got = self.s.centroidal(matrix=matrix, bias=bias, out=st, out_matrix=mt, out_bias=bt)
        assert got.state is st and got.matrix is (mt if matrix else None) and got.bias is (bt if bias else None)
        torch.cuda.synchronize()
        return st.cpu().numpy(), mt.cpu().numpy(), bt.cpu().numpy()

    def figures(self, st, A, b):
        """max |got - ref| / max |ref| per block, over all envs and for the far env alone."""
        rs, rA, rb = self.ref_state, self.ref_A, self.ref_bias
        rootp = self.root[:, :3].astype(np.float64)
        pairs = {"c_rel": (st[:, :3].astype(np.float64) - rootp, rs[:, :3] - rootp, None),
                 "cdot": (st[:, 3:6], rs[:, 3:6], rs[:, 3:9]), "k": (st[:, 6:9], rs[:, 6:9], rs[:, 3:9]),
                 "M": (st[:, 9], rs[:, 9], None), "IG": (st[:, 10:], rs[:, 10:], None),
                 "A_lin": (A[:, :3], rA[:, :3], rA), "A_ang": (A[:, 3:], rA[:, 3:], rA),
                 "bias_lin": (b[:, :3], rb[:, :3], rb), "bias_ang": (b[:, 3:], rb[:, 3:], rb)}
        # (c_rel: what is left of |c - c_ref| beyond one fp32 ulp of the absolute coordinate, the module docstring's rule)
        ulp = np.spacing(np.abs(rs[:, :3]).astype(np.float32)).astype(np.float64)
        excess = np.maximum(np.abs(st[:, :3].astype(np.float64) - rs[:, :3]) - ulp, 0.0)
        pairs["c_rel"] = (pairs["c_rel"][1] + excess, pairs["c_rel"][1], None)
        fig, far = {}, {}
        for name, (g, r, whole) in pairs.items():
            scale = float(np.abs(r).max())
            if whole is not None and scale <= 1e-6 * float(np.abs(whole).max()):
                scale = float(np.abs(whole).max())      # a block that is identically zero (the single body)
            if scale == 0.0:
                scale = 1.0
            fig[name] = float(np.abs(g - r).max()) / scale
            if self.n > 1:
                far[name] = float(np.abs(g[1] - r[1]).max()) / scale
        return fig, far

    def check(self, st, A, b, what):
        assert st.dtype == A.dtype == b.dtype == np.float32
        assert not (np.isnan(st).any() or np.isnan(A).any() or np.isnan(b).any())     # every element is written
        fig, far = self.figures(st, A, b)
        print({"case": self.case, "n": self.n, "what": what, "blocks": fig, "far_env": far})
        for name in BLOCKS:
            assert fig[name] <= self.tol, (name, fig)
            if self.n > 1:
                assert far[name] <= self.tol, (name, far)
        # state[0:3] itself: the relative com at the tolerance, plus one fp32 ulp of the absolute coordinate
        cref = self.ref_state[:, :3]
        arm = float(np.abs(cref - self.root[:, :3].astype(np.float64)).max())
        ulp = np.spacing(np.abs(cref).astype(np.float32)).astype(np.float64)
        assert (np.abs(st[:, :3].astype(np.float64) - cref) <= self.tol * arm + ulp).all(), fig
        return fig


_cases = {}


def shared(case):
    """One shared Case per model with the four call forms made, read-only."""
    if case not in _cases:
        c = Case(case)
        c.got = {k: c.call(*v) for k, v in FORMS.items()}
        _cases[case] = c
    return _cases[case]


@pytest.mark.parametrize("case", CASES)
def test_outputs_match_the_reference(case):
    c = shared(case)
    c.check(*c.got["all"], "all three")
    assert float(np.abs(c.ref_state[:, 6:9]).max()) > 1e-2 and float(np.abs(c.ref_bias).max()) > 1e-2


@pytest.mark.parametrize("case", ["thormang", "gogoro", "kat_free"])
def test_one_env(case):
    c = Case(case, n=1, seed=42)
    c.check(*c.call(True, True), "one env")


def test_runtime_loaded_model():
    """jit_walker is compiled at run time (tg_model_jit): the call works, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = shared("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()


@pytest.mark.parametrize("case", CASES)
def test_exact_blocks(case):
    """A[0:3, 0:3] = M 1 and A[3:6, 0:3] = 0, bit for bit, M the state's."""
    c = shared(case)
    st, A, _b = c.got["all"]
    for e in range(N):
        want = np.zeros((6, 3), np.float32)
        want[0, 0] = want[1, 1] = want[2, 2] = st[e, 9]
        assert np.array_equal(A[e, :, :3].view(np.uint32), want.view(np.uint32)), (e, A[e, :, :3])
    assert (st[:, 9] > 0).all()


@pytest.mark.parametrize("case", CASES)
def test_call_forms_agree_bit_for_bit_and_leave_other_buffers_alone(case):
    c = shared(case)
    st, A, b = c.got["all"]
    for form, (matrix, bias) in FORMS.items():
        s2, A2, b2 = c.got[form]
        assert np.array_equal(s2.view(np.uint32), st.view(np.uint32)), form
        if matrix:
            assert np.array_equal(A2.view(np.uint32), A.view(np.uint32)), form
        else:
            assert np.isnan(A2).all(), form                               # not requested: still all NaN
        if bias:
            assert np.array_equal(b2.view(np.uint32), b.view(np.uint32)), form
        else:
            assert np.isnan(b2).all(), form
    # matrix or bias without the state, through the C ABI: the state buffer is not touched
    from thormang_isaacgym_amd._lib import lib
    st3, A3, b3 = _nan(N, 16), _nan(N, 6, 6 + c.D), _nan(N, 6)
    assert lib().tg_centroidal(c.s.handle, None, A3.data_ptr(), None) == 0
    assert lib().tg_centroidal(c.s.handle, None, None, b3.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(A3.cpu().numpy().view(np.uint32), A.view(np.uint32))
    assert np.array_equal(b3.cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert bool(torch.isnan(st3).all())
    # without out tensors the sim's own come back, with the same values; parts not asked for are None
    own = c.s.centroidal(matrix=True, bias=True)
    torch.cuda.synchronize()
    assert np.array_equal(own.state.cpu().numpy(), st) and np.array_equal(own.matrix.cpu().numpy(), A)
    assert np.array_equal(own.bias.cpu().numpy(), b)
    only = c.s.centroidal()
    assert only.state is own.state and only.matrix is None and only.bias is None


@pytest.mark.parametrize("case", CASES)
def test_identities_on_the_gpu_tensors(case):
    """A u against the state; A against the base rows of the mass-matrix tensor (tg_mass_matrices, the kernel of
    refresh_mass_matrix_tensors) moved to the com; the bias
    against the base rows of inverse_dynamics(gravity=False) moved to the com."""
    c = shared(case)
    s = c.s
    st, A, b = (x.astype(np.float64) for x in c.got["all"])
    h = np.concatenate([st[:, 9:10] * st[:, 3:6], st[:, 6:9]], axis=1)
    Au = np.einsum("eij,ej->ei", A, c.u)
    d1 = float(np.abs(Au - h).max() / np.abs(h).max())
    from thormang_isaacgym_amd._lib import lib
    H = _nan(N, 6 + c.D, 6 + c.D)             # (the full layout with fix_base too, where the sim's own tensor is a view)
    assert lib().tg_mass_matrices(s.handle, H.data_ptr()) == 0
    tau = s.inverse_dynamics(gravity=False)
    torch.cuda.synchronize()
    H, tau = H.double().cpu().numpy(), tau.double().cpu().numpy()
    lever = c.c_rel - c.kin.c[:, 0]                                        # c - c_root
    wantA = np.concatenate([H[:, :3], H[:, 3:6] - np.cross(lever[:, :, None], H[:, :3], axisa=1, axisb=1, axisc=1)],
                           axis=1)
    d2 = float(np.abs(A - wantA).max() / np.abs(wantA).max())
    wantb = np.concatenate([tau[:, :3], tau[:, 3:6] - np.cross(lever, tau[:, :3])], axis=1)
    d3 = float(np.abs(b - wantb).max() / np.abs(wantb).max())
    print({"case": case, "Au_vs_state": d1, "A_vs_mass_matrix": d2, "bias_vs_inverse_dynamics": d3})
    assert d1 <= c.tol and d2 <= c.tol and d3 <= c.tol


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_moving_the_env_changes_only_the_com_position(case):
    c = shared(case)
    s = c.s
    far = c.got["all"]
    root0 = s.root_state.clone()
    try:
        s.root_state[1, :3] = 0.0
        near = c.call(True, True)
    finally:
        s.root_state.copy_(root0)
    for f, g in zip(far, near):
        assert f.shape == g.shape
    assert np.array_equal(far[0][:, 3:].view(np.uint32), near[0][:, 3:].view(np.uint32))
    assert np.array_equal(far[1].view(np.uint32), near[1].view(np.uint32))
    assert np.array_equal(far[2].view(np.uint32), near[2].view(np.uint32))
    others = [e for e in range(N) if e != 1]
    assert np.array_equal(far[0][others].view(np.uint32), near[0][others].view(np.uint32))
    assert np.abs(far[0][1, :3] - near[0][1, :3] - np.asarray(FAR)).max() <= 1e-4      # (and the com went with it)
    again = c.call(True, True)                                                         # (restored)
    assert all(np.array_equal(x, y) for x, y in zip(again, far))


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_the_sim_is_unchanged(case):
    c = shared(case)
    s = c.s
    before = [t.clone() for t in (s.root_state, s.dof_state, s.dof_pos_target, s.dof_vel_target, s.dof_actuation,
                                  s.dof_props)]
    c.call(True, True)
    after = (s.root_state, s.dof_state, s.dof_pos_target, s.dof_vel_target, s.dof_actuation, s.dof_props)
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(s.root_state.cpu().numpy(), c.root) and np.array_equal(s.dof_state.cpu().numpy(), c.dof)


def test_mass_scale_and_velocity_enter():
    """A reference without the env's mass scales lies more than 10 x the tolerance away."""
    c = shared("thormang")
    plain = state_ref(c.m, c.root, c.dof, None, c.kin.desc)
    d = float(np.abs(plain[:, 3:] - c.ref_state[:, 3:]).max() / np.abs(c.ref_state[:, 3:]).max())
    assert d > 10 * c.tol, d


def test_walk_task_exposes_the_centroidal_state_and_is_otherwise_unchanged():
    """ThormangWalk, 16 envs, 20 steps of fixed actions, env.enableCentroidalState on against off: obs, reward and
    reset bit-identical; extras["centroidal"] is sim.centroidal().state of the state the step returned with."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_cfg
    n = 16
    envs = []
    for on in (False, True):
        cfg = walk_cfg(n)
        if on:
            cfg["env"]["enableCentroidalState"] = True
        envs.append(make_gpu_walk(cfg, NumpyDraws(5)))
    off, on = envs
    D = on.model.num_dof
    assert off.centroidal_state is None and "centroidal" not in off.extras
    act = torch.from_numpy(np.random.default_rng(9).uniform(-0.5, 0.5, (n, D)).astype(np.float32)).cuda()
    seen = 0.0
    for _ in range(20):
        o0, r0, z0, x0 = off.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        assert torch.equal(o0["obs"], o1["obs"]) and torch.equal(r0, r1) and torch.equal(z0, z1)
        assert torch.equal(x0["time_outs"], x1["time_outs"]) and "centroidal" not in x0
        cen = x1["centroidal"]
        assert tuple(cen.shape) == (n, 16) and bool(torch.isfinite(cen).all())
        kept = cen.clone()
        assert torch.equal(on.sim.centroidal().state, kept) and torch.equal(on.centroidal().state, kept)
        seen = max(seen, float(cen[:, 3:9].abs().max()))
    assert torch.equal(off.sim.root_state, on.sim.root_state) and torch.equal(off.sim.dof_state, on.sim.dof_state)
    assert seen > 0 and bool((cen[:, 2] > 0.1).all()) and bool((cen[:, 9] > 10).all())


def test_error_paths():
    from thormang_isaacgym_amd._lib import lib
    c = shared("thormang")
    s, D = c.s, c.D
    assert lib().tg_centroidal(s.handle, None, None, None) == -1           # TG_ERR_ARG
    assert lib().tg_last_error().startswith(b"tg_centroidal:")
    assert lib().tg_centroidal(None, None, None, None) == -1
    assert lib().tg_last_error().startswith(b"tg_centroidal:")
    with pytest.raises(ValueError):
        s.centroidal(out=torch.zeros(N, 15, device="cuda:0"))               # shape
    with pytest.raises(ValueError):
        s.centroidal(out=torch.zeros(N, 16, device="cuda:0").double())      # dtype
    with pytest.raises(ValueError):
        s.centroidal(out=torch.zeros(N, 16))                                # device
    with pytest.raises(ValueError):
        s.centroidal(out=torch.zeros(16, N, device="cuda:0").t())           # contiguity
    with pytest.raises(ValueError):
        s.centroidal(matrix=True, out_matrix=torch.zeros(N, 6 + D, 6, device="cuda:0"))
    with pytest.raises(ValueError):
        s.centroidal(out_bias=torch.zeros(N, 3, device="cuda:0"))              # checked even when not requested
    torch.cuda.synchronize()
