"""Jacobian and mass-matrix tensors on the GPU (tg_jacobians / tg_mass_matrices,
Sim.acquire/refresh_jacobian_tensors, acquire/refresh_mass_matrix_tensors)
against the float64 reference built from the oracle (tests/jacobian_ref.py).

Five envs (no multiple of anything), thormang and gogoro (locked and prismatic
DOFs, depth 12): random states, env 1 far out on the grid at (300, -200, 1),
random mass scales in [0.9, 1.1] and armatures in [0, 0.05], the output
tensors filled with NaN before each refresh.

Mass-matrix tolerance: max |H - H_ref| per env <= tol x that env's largest
reference diagonal entry, tol = 4 x the worst ratio measured on the MI355X
over the states these tests use (hard cap 1e-4; a dropped link or a wrong
lever arm shows at 1e-2 or more).  Measured worst ratios (H_MEASURED below):
thormang 7.5e-8, gogoro 1.9e-7, jit_walker 1.0e-7 with a floating base; with
a fixed base, where the scale is the joint block's largest diagonal entry and
no longer the body's mass, the pendulum 2.2e-7 and thormang 5.6e-7.  All of
it float32 rounding: the float32 evaluation of the reference sum itself
differs from float64 by up to 2e-7 of that scale."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.jacobian_ref import ancestor_columns, jacobian_ref, mass_matrix_ref
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

N = 5
FAR = (300.0, -200.0, 1.0)
J_ATOL = 6e-5     # twice the 3e-5 position tolerance of test_gpu_rigid_body_states_match_oracle
# worst measured ratio per (model, fixed base); the tolerance is 4 x it, hard cap 1e-4
H_MEASURED = {("thormang", False): 7.6e-8, ("gogoro", False): 1.95e-7, ("jit_walker", False): 1.02e-7,
              ("pendulum", True): 2.3e-7, ("thormang", True): 5.7e-7}
assert 4 * max(H_MEASURED.values()) <= 1e-4


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return {"pendulum": pm.pendulum, "jit_walker": pm.jit_walker}.get(name, lambda: load_model(name))()


def nan_fill(s):
    s._jacobian.fill_(float("nan"))
    s._mass_matrix.fill_(float("nan"))


class Case:
    """A sim of ``n`` envs in the test state, refreshed once, with its references."""

    def __init__(self, name, n=N, fix_base=False, seed=17):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.m = m = _model(name)
        self.h_tol = 4 * H_MEASURED[(name, fix_base)] if (name, fix_base) in H_MEASURED else None
        self.n, self.L, self.D = n, m.num_bodies, m.num_dof
        rs = np.random.default_rng(seed)
        self.root, self.dof = random_state(m, n, rs)
        if n > 1:
            self.root[1, :3] = FAR
        self.ms = rs.uniform(0.9, 1.1, (n, self.L)).astype(np.float32)
        self.arm = rs.uniform(0.0, 0.05, (n, self.D)).astype(np.float32)
        kw = dict(fix_base_link=True) if fix_base else {}
        sp = pm.sim(m, n=n, dt=0.01, substeps=1, **kw)[1]
        self.s = s = Sim(m, sp, n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        ids = torch.arange(n, device="cuda:0")
        s.set_body_mass_scale_indexed(torch.from_numpy(self.ms).cuda(), ids)
        s.set_dof_properties_indexed(abi.TG_PROP_ARMATURE, torch.from_numpy(self.arm).cuda(), ids)
        self.Jt, self.Ht = s.acquire_jacobian_tensor(), s.acquire_mass_matrix_tensor()
        self.refresh()
        self.reference()

    def refresh(self):
        nan_fill(self.s)
        self.s.refresh_jacobian_tensors()
        self.s.refresh_mass_matrix_tensors()
        torch.cuda.synchronize()
        self.J, self.H = self.Jt.cpu().numpy(), self.Ht.cpu().numpy()
        self.Jfull, self.Hfull = self.s._jacobian.cpu().numpy(), self.s._mass_matrix.cpu().numpy()

    def reference(self):
        self.J_ref = jacobian_ref(self.m, self.root, self.dof)
        self.H_ref = mass_matrix_ref(self.m, self.root, self.dof, self.ms, self.arm, J=self.J_ref)

    def h_ratio(self, H=None, H_ref=None):
        """worst over the envs of max |H - H_ref| / the env's largest reference diagonal entry"""
        H = self.Hfull if H is None else H
        H_ref = self.H_ref if H_ref is None else H_ref
        if not np.isfinite(H).all():
            return float("inf")
        diag = np.diagonal(H_ref, axis1=1, axis2=2).max(axis=1)
        return float((np.abs(H - H_ref).reshape(self.n, -1).max(axis=1) / diag).max())


_cases = {}


@pytest.fixture(params=["thormang", "gogoro"])
def case(request):
    """One shared, read-only Case per model."""
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def test_every_element_is_written(case):
    assert case.Jfull.shape == (N, case.L, 6, case.D + 6) and case.Hfull.shape == (N, case.D + 6, case.D + 6)
    assert not np.isnan(case.Jfull).any()
    assert not np.isnan(case.Hfull).any()


def test_jacobian_matches_the_reference(case):
    err = float(np.abs(case.Jfull - case.J_ref).max())
    far = float(np.abs(case.Jfull[1] - case.J_ref[1]).max())
    print({"model": case.m.name, "J_max_abs_err": err, "far_env_err": far, "max_abs_J": float(np.abs(case.J_ref).max())})
    np.testing.assert_allclose(case.Jfull, case.J_ref, rtol=0, atol=J_ATOL)


def test_jacobian_exact_structure(case):
    J = case.Jfull
    mask = ancestor_columns(case.m)                       # [L, 6 + D]
    off = np.broadcast_to(~mask[None, :, None, :], J.shape)
    assert (J[off] == 0.0).all()
    assert mask.sum() < mask.size                          # (the pattern is not trivial)
    assert (J[:, :, :3, :3] == np.eye(3, dtype=np.float32)).all()
    assert (J[:, :, 3:, :3] == 0.0).all()


def test_jacobian_times_u_is_the_rigid_body_velocity(case):
    s = case.s
    rb = s.acquire_rigid_body_state_tensor()
    s.refresh_rigid_body_state_tensor()
    u = torch.cat([s.root_state[:, 7:13], s.dof_state.view(N, case.D, 2)[:, :, 1]], dim=1)
    v = torch.einsum("nlrc,nc->nlr", s._jacobian, u).cpu().numpy()
    np.testing.assert_allclose(v, rb.view(N, case.L, 13)[..., 7:13].cpu().numpy(), atol=2e-4, rtol=1e-4)


def test_mass_matrix_matches_the_reference(case):
    ratio = case.h_ratio()
    print({"model": case.m.name, "H_worst_ratio": ratio,
           "max_diag": float(np.diagonal(case.H_ref, axis1=1, axis2=2).max())})
    assert ratio <= case.h_tol, ratio


def test_mass_matrix_is_symmetric_bit_for_bit(case):
    H = case.s._mass_matrix
    assert torch.equal(H, H.transpose(1, 2))


def test_mass_matrix_is_positive_definite(case):
    for e in range(N):
        lo = float(np.linalg.eigvalsh(case.Hfull[e].astype(np.float64)).min())
        assert lo > 0.0, (e, lo)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_second_refresh_changes_only_the_env_that_moved(name):
    c = Case(name)
    J0, H0 = c.Jfull.copy(), c.Hfull.copy()
    rs = np.random.default_rng(5)
    dof = c.dof.reshape(N, c.D, 2).copy()
    dof[2, :, 0] = rs.uniform(-1, 1, c.D)
    c.s.set_dof_state_indexed(torch.from_numpy(dof.reshape(N * c.D, 2)).cuda(),
                              torch.tensor([2], dtype=torch.int32, device="cuda:0"))
    c.refresh()
    keep = [0, 1, 3, 4]
    assert np.array_equal(c.Jfull[keep], J0[keep]) and np.array_equal(c.Hfull[keep], H0[keep])
    assert not np.array_equal(c.Jfull[2], J0[2]) and not np.array_equal(c.Hfull[2], H0[2])
    c.dof = np.ascontiguousarray(dof.reshape(N * c.D, 2))
    c.reference()
    np.testing.assert_allclose(c.Jfull, c.J_ref, rtol=0, atol=J_ATOL)
    print({"model": c.m.name, "second_refresh_H_worst_ratio": c.h_ratio()})
    assert c.h_ratio() <= c.h_tol


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_one_env(name):
    c = Case(name, n=1)
    assert not np.isnan(c.Jfull).any() and not np.isnan(c.Hfull).any()
    np.testing.assert_allclose(c.Jfull, c.J_ref, rtol=0, atol=J_ATOL)
    print({"model": c.m.name, "one_env_H_worst_ratio": c.h_ratio()})
    assert c.h_ratio() <= c.h_tol


@pytest.mark.parametrize("name", ["pendulum", "thormang"])
def test_fixed_base_views(name):
    """IsaacGym's fixed-base rule: no root link, no base rows or columns."""
    c = Case(name, fix_base=True)
    assert tuple(c.Jt.shape) == (N, c.L - 1, 6, c.D) and tuple(c.Ht.shape) == (N, c.D, c.D)
    assert c.Jt.data_ptr() == c.s._jacobian[:, 1:, :, 6:].data_ptr()       # views of the same storage
    assert c.Ht.data_ptr() == c.s._mass_matrix[:, 6:, 6:].data_ptr()
    assert not np.isnan(c.Jfull).any() and not np.isnan(c.Hfull).any()
    np.testing.assert_allclose(c.J, c.J_ref[:, 1:, :, 6:], rtol=0, atol=J_ATOL)
    ratio = c.h_ratio(c.H, c.H_ref[:, 6:, 6:])
    print({"model": c.m.name, "fixed_base_H_worst_ratio": ratio})
    assert ratio <= c.h_tol, ratio


def test_runtime_loaded_model():
    """A model compiled at run time (tg_model_jit): both calls work, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = Case("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()
    assert not np.isnan(c.Jfull).any() and not np.isnan(c.Hfull).any()
    np.testing.assert_allclose(c.Jfull, c.J_ref, rtol=0, atol=J_ATOL)
    mask = ancestor_columns(c.m)
    assert (c.Jfull[np.broadcast_to(~mask[None, :, None, :], c.Jfull.shape)] == 0.0).all()
    ratio = c.h_ratio()
    print({"model": c.m.name, "H_worst_ratio": ratio})
    assert ratio <= c.h_tol, ratio
    assert torch.equal(c.s._mass_matrix, c.s._mass_matrix.transpose(1, 2))


def test_null_output_is_an_argument_error():
    from thormang_isaacgym_amd._lib import lib
    c = Case("pendulum", n=1)
    for f, what in ((lib().tg_jacobians, b"tg_jacobians"), (lib().tg_mass_matrices, b"tg_mass_matrices")):
        assert f(c.s.handle, None) == -1   # TG_ERR_ARG
        assert what in lib().tg_last_error()
    _ = C
