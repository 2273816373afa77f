"""Inverse dynamics on the GPU (tg_inverse_dynamics, Sim.inverse_dynamics)
against the float64 reference built from the oracle (tests/id_ref.py, pinned by
tests/test_id_reference.py).

Five envs (no multiple of anything), env 1 far out on the grid at
(300, -200, 1), random root pose, random root and joint velocities, every sim
with a body mass scale U(0.8, 1.2) per link and an armature U(0.005, 0.02) per
DOF, the output tensor filled with NaN before each call.

Tolerance.  max |tau - tau_ref| / max |tau_ref| per comparison, <= 4 x the
worst value measured on the MI355X on this file's first run (ID_MEASURED
below, per model), under the project's hard cap of 1e-4 relative, asserted.
The far env is held to the same bound.  The identities against the Jacobian
and mass-matrix tensors take the same bound on the same scale.  Measured:
thormang 1.9e-7 (velocity only, the far env), gogoro 1.5e-7, the run-time
jit_walker 1.4e-7; the identities 8.7e-8 and 1.1e-7."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.id_ref import GRAVITY, Kinematics, efforts_ref, id_ref
from tests.ik_ref import chain_spec, pose_error
from tests.test_id_reference import (CLOSED_LOOP_N, CLOSED_LOOP_STEPS, COAST_BOUND, FAR, HOLD_BOUND, closed_loop_case,
                                     reference_loop)
from tests.test_osc_reference import CLOSED_LOOP_CASES, CLOSED_LOOP_DAMPING, KP, KP_NULL
from tests.test_osc_reference import CLOSED_LOOP_STEPS as OSC_STEPS
from tests.test_osc_reference import closed_loop_case as osc_closed_loop_case
from tests.test_osc_reference import error_norms
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

N = 5
MODELS = ["thormang", "gogoro", "jit_walker"]
# (gravity, velocity, accel)
TERMS = {"gravity": (True, False, False), "velocity": (False, True, False), "both": (True, True, False),
         "both_accel": (True, True, True)}
# worst max |tau - tau_ref| / max |tau_ref| per model, measured on the MI355X over every comparison
# in this file; the tolerance is 4 x it
ID_MEASURED = {"thormang": 2.0e-7, "gogoro": 1.6e-7, "jit_walker": 1.5e-7}
assert 4 * max(ID_MEASURED.values()) <= 1e-4


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return pm.jit_walker() if name == "jit_walker" else load_model(name)


class Case:
    """A sim of ``n`` envs in the test state with the reference's inputs; ``call`` runs one call on a NaN-filled output."""

    def __init__(self, name, n=N, seed=31, fix_base=False):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.name, self.m, self.n = name, _model(name), n
        m = self.m
        self.D, self.L = D, L = m.num_dof, m.num_bodies
        rs = np.random.default_rng(seed)
        self.root, self.dof = random_state(m, n, rs)
        if n > 1:
            self.root[1, :3] = FAR
        if fix_base:
            self.root[:, 7:13] = 0.0
        self.ms = rs.uniform(0.8, 1.2, (n, L)).astype(np.float32)
        self.arm = rs.uniform(0.005, 0.02, (n, D)).astype(np.float32)
        self.accel = rs.normal(0, 2.0, (n, 6 + D)).astype(np.float32)
        ao = dict(fix_base_link=True) if fix_base else {}
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1, **ao)[1], n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        s.set_body_mass_scale_indexed(torch.from_numpy(self.ms).cuda(), torch.arange(n, device="cuda:0"))
        props = abi.default_dof_props(m, n)
        props[abi.TG_PROP_ARMATURE] = self.arm
        s.dof_props.copy_(torch.from_numpy(props))
        s.refresh()
        self.effort = s.dof_props[abi.TG_PROP_EFFORT].cpu().numpy()
        self.accel_t = torch.from_numpy(self.accel).cuda()
        self.kin = Kinematics(m, self.root, self.dof)
        self.tol = 4 * ID_MEASURED[name]

    def call(self, gravity=True, velocity=True, accel=False, **kw):
        out = torch.full((self.n, 6 + self.D), float("nan"), dtype=torch.float32, device="cuda:0")
        got = self.s.inverse_dynamics(accel=self.accel_t if accel else None, gravity=gravity, velocity=velocity,
                                      out=out, **kw)
        assert got is out
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def reference(self, gravity=True, velocity=True, accel=False, mass_scale=True, armature=True, g=GRAVITY):
        return id_ref(self.m, self.root, self.dof, accel=self.accel if accel else None, gravity=gravity,
                      velocity=velocity, g=g, mass_scale=self.ms if mass_scale else None,
                      armature=self.arm if armature else None, kin=self.kin)

    def check(self, tau, ref, what):
        assert tau.shape == (self.n, 6 + self.D) and tau.dtype == np.float32
        assert not np.isnan(tau).any()                                      # every element is written
        scale = float(np.abs(ref).max())
        fig = {"model": self.name, "what": what, "tau_rel": float(np.abs(tau - ref).max()) / scale,
               "dof_rows_rel": float(np.abs(tau[:, 6:] - ref[:, 6:]).max()) / scale, "max_abs_tau": scale}
        if self.n > 1:
            others = [e for e in range(self.n) if e != 1]
            fig["far_env"] = float(np.abs(tau[1] - ref[1]).max()) / scale
            fig["other_envs"] = float(np.abs(tau[others] - ref[others]).max()) / scale
        print(fig)
        assert fig["tau_rel"] <= self.tol, fig
        if self.n > 1:
            assert fig["far_env"] <= self.tol, fig
        return fig


_cases = {}


def shared(name):
    """One shared Case per model with the four calls made and their references computed, read-only."""
    if name not in _cases:
        c = Case(name)
        c.got = {k: c.call(*v) for k, v in TERMS.items()}
        c.ref = {k: c.reference(*v) for k, v in TERMS.items()}
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("terms", list(TERMS))
@pytest.mark.parametrize("name", MODELS)
def test_tau_matches_the_reference(name, terms):
    c = shared(name)
    c.check(c.got[terms], c.ref[terms], terms)
    # (the four results differ: no call answered for another)
    for other in TERMS:
        if other != terms:
            assert np.abs(c.ref[other] - c.ref[terms]).max() > 1e-2 * np.abs(c.ref[terms]).max()


def test_runtime_loaded_model():
    """jit_walker is compiled at run time (tg_model_jit): the call works, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = shared("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()


def test_the_sims_current_gravity_is_used():
    c = shared("thormang")
    g = (0.3, -0.2, -9.0)
    c.s.set_gravity(g)
    try:
        tau = c.call(True, True, False)
    finally:
        c.s.set_gravity(GRAVITY)
    c.check(tau, c.reference(True, True, False, g=g), "set_gravity")
    assert np.abs(tau - c.got["both"]).max() > 1e-2 * np.abs(c.got["both"]).max()
    assert np.array_equal(c.call(True, True, False), c.got["both"])         # (and restored)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_identities_on_the_jacobian_and_mass_matrix_tensors(name):
    """Gravity-only tau = -sum_l s_l m_l Jv_l^T g over acquire_jacobian_tensor();
    tau(a) - tau(0) = acquire_mass_matrix_tensor() @ a."""
    c = shared(name)
    s = c.s
    J = s.acquire_jacobian_tensor()
    s.refresh_jacobian_tensors()
    H = s.acquire_mass_matrix_tensor()
    s.refresh_mass_matrix_tensors()
    torch.cuda.synchronize()
    assert tuple(J.shape) == (N, c.L, 6, 6 + c.D) and tuple(H.shape) == (N, 6 + c.D, 6 + c.D)
    mass = torch.from_numpy(np.asarray(abi.model_arrays(c.m)["link_inertia"], np.float64)[:, 0])
    w = torch.from_numpy(c.ms.astype(np.float64)) * mass[None, :]                                  # [N, L]
    g = torch.tensor(GRAVITY, dtype=torch.float64)
    want = -torch.einsum("el,elkc,k->ec", w, J[:, :, :3].double().cpu(), g).numpy()
    scale = float(np.abs(c.ref["gravity"]).max())
    d1 = float(np.abs(c.got["gravity"] - want).max()) / scale
    Ha = torch.einsum("eij,ej->ei", H.double().cpu(), torch.from_numpy(c.accel.astype(np.float64))).numpy()
    scale2 = float(np.abs(c.ref["both_accel"]).max())
    d2 = float(np.abs((c.got["both_accel"].astype(np.float64) - c.got["both"]) - Ha).max()) / scale2
    only = c.call(False, False, True)                                        # terms == 0 with accel: H a alone
    d3 = float(np.abs(only - Ha).max()) / float(np.abs(Ha).max())
    print({"model": name, "gravity_vs_jacobian_sum": d1, "accel_vs_mass_matrix": d2, "accel_alone": d3})
    assert d1 <= c.tol and d2 <= c.tol and d3 <= c.tol


@pytest.mark.parametrize("name", MODELS)
def test_mass_scale_armature_and_velocity_enter(name):
    """A reference without the env's mass scale or without the velocity term
    lies more than 10 x the tolerance away, and so does one without its
    armature, judged on H a alone."""
    c = shared(name)
    ref = c.ref["both_accel"]
    scale = float(np.abs(ref).max())
    for what, r in (("no mass scale", c.reference(True, True, True, mass_scale=False)),
                    ("no velocity term", c.reference(True, False, True))):
        d = float(np.abs(r - ref).max()) / scale
        print({"model": name, "reference": what, "tau_rel_change": d})
        assert d > 10 * c.tol, (what, d)
    ha = c.reference(False, False, True)
    d = float(np.abs(c.reference(False, False, True, armature=False) - ha).max() / np.abs(ha).max())
    got = c.call(False, False, True)
    e = float(np.abs(got - ha).max() / np.abs(ha).max())
    print({"model": name, "reference": "no armature, H a alone", "tau_rel_change": d, "kernel_error": e})
    assert e <= c.tol and d > 10 * c.tol, (d, e)


def test_locked_and_prismatic_dofs_get_their_entries():
    """gogoro: the arm DOFs are locked and base_y is prismatic and locked: ordinary entries."""
    c = shared("gogoro")
    by = c.m.dof_names.index("base_y")
    locked = sorted(set(c.m.locked_dofs))
    assert by in locked and len(locked) > 7
    tau, ref = c.got["both"], c.ref["both"]
    scale = float(np.abs(ref).max())
    assert (np.abs(ref[:, 6 + by]) > 1e-2).all()
    assert (np.abs(ref[:, [6 + d for d in locked]]).max(axis=0) > 1e-4).all()
    assert np.abs(tau[:, [6 + d for d in locked]] - ref[:, [6 + d for d in locked]]).max() <= c.tol * scale
    # the prismatic entry is the force along the axis: with gravity alone and no velocity it is the
    # weight of the subtree on the axis, which the float32 kernel reproduces
    assert np.abs(c.got["gravity"][:, 6 + by] - c.ref["gravity"][:, 6 + by]).max() <= c.tol * scale


def test_fix_base_writes_the_full_layout():
    c = Case("thormang", fix_base=True)
    assert c.s.params.fix_base
    tau = c.call(True, True, True)
    ref = c.reference(True, True, True)
    c.check(tau, ref, "fix_base")
    assert (np.abs(tau[:, :6]).max(axis=0) > 1e-2).all()                    # the reaction at the base


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_state_is_unchanged_and_calls_repeat_bit_for_bit(name):
    c = shared(name)
    s = c.s
    root0, dof0 = s.root_state.clone(), s.dof_state.clone()
    props0, act0 = s.dof_props.clone(), s.dof_actuation.clone()
    eff = torch.zeros(N, c.D, dtype=torch.float32, device="cuda:0")
    a = c.call(True, True, True, efforts=eff)
    b = c.call(True, True, True, efforts=eff.clone())
    assert np.array_equal(a, b) and np.array_equal(a, c.got["both_accel"])
    assert torch.equal(s.root_state, root0) and torch.equal(s.dof_state, dof0)
    assert torch.equal(s.dof_props, props0) and torch.equal(s.dof_actuation, act0)
    assert np.array_equal(root0.cpu().numpy(), c.root) and np.array_equal(dof0.cpu().numpy(), c.dof)
    assert torch.equal(c.accel_t.cpu(), torch.from_numpy(c.accel))
    # without ``out`` the sim's own tensor comes back, with the same values
    own = s.inverse_dynamics(accel=c.accel_t)
    torch.cuda.synchronize()
    assert own is s.inverse_dynamics(accel=c.accel_t) and np.array_equal(own.cpu().numpy(), a)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_one_env(name):
    c = Case(name, n=1, seed=32)
    c.check(c.call(True, True, True), c.reference(True, True, True), "one env")


def test_efforts():
    """Overwrite against accumulate, the clamp at a deliberately small effort
    limit, DOF selection by name and by index, and a sentinel in every element
    that is not selected."""
    c = Case("thormang")
    s, D = c.s, c.D
    names = ["l_arm_sh_p1", "l_arm_sh_r", "l_arm_el_y", "r_leg_kn_p", "torso_y"]
    idx = [c.m.dof_names.index(x) for x in names]
    ref = c.reference(True, True, False)
    low = idx[int(np.argmax(np.abs(ref[:, [6 + d for d in idx]]).min(axis=0)))]
    lim = np.float32(0.5 * np.abs(ref[:, 6 + low]).min())
    assert lim > 1e-3
    s.dof_props[abi.TG_PROP_EFFORT][:, low] = float(lim)
    s.refresh()
    effort = s.dof_props[abi.TG_PROP_EFFORT].cpu().numpy()
    sentinel = torch.arange(N * D, dtype=torch.float32, device="cuda:0").reshape(N, D) * 0.5 + 1000.0
    sel = np.zeros(D, bool)
    sel[idx] = True
    # overwrite, by name
    eff = sentinel.clone()
    tau = c.call(True, True, False, dofs=names, efforts=eff)
    got = eff.cpu().numpy()
    assert np.array_equal(got[:, ~sel], sentinel.cpu().numpy()[:, ~sel])
    expect = np.clip(tau[:, 6:], -effort, effort)
    assert np.array_equal(got[:, sel], expect[:, sel])
    assert set(np.abs(got[:, low]).tolist()) == {float(lim)}                 # the clamp acts in every env
    others = [d for d in idx if d != low]
    assert (np.abs(tau[:, [6 + d for d in others]]) < effort[:, others]).all()   # (and nowhere else)
    ref64 = efforts_ref(ref, effort, sentinel.cpu().numpy(), idx)
    np.testing.assert_allclose(got, ref64, rtol=0, atol=c.tol * np.abs(ref).max())
    # by index: the same
    eff2 = sentinel.clone()
    c.call(True, True, False, dofs=idx, efforts=eff2)
    assert torch.equal(eff2, eff)
    # accumulate on a base of its own
    base = (torch.arange(N * D, dtype=torch.float32, device="cuda:0").reshape(N, D) % 7 - 3.0) * 0.25
    eff3 = base.clone()
    c.call(True, True, False, dofs=idx, efforts=eff3, accumulate=True)
    got3, b = eff3.cpu().numpy(), base.cpu().numpy()
    assert np.array_equal(got3[:, ~sel], b[:, ~sel])
    np.testing.assert_allclose(got3[:, sel], np.clip(b + tau[:, 6:], -effort, effort)[:, sel], rtol=1e-6, atol=1e-7)
    assert np.abs(got3[:, others] - got[:, others]).max() > 0.1              # (accumulate is not overwrite)
    assert (np.abs(got3[:, low]) <= lim).all()
    # every DOF (dofs=None), efforts alone through the C ABI
    from thormang_isaacgym_amd._lib import lib
    eff4 = sentinel.clone()
    assert lib().tg_inverse_dynamics(s.handle, 3, None, None, eff4.data_ptr(), None, 0, 0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(eff4.cpu().numpy(), expect)


def test_argument_errors():
    """Every argument error of the header returns TG_ERR_ARG with tg_inverse_dynamics in the message."""
    from thormang_isaacgym_amd._lib import lib
    c = shared("thormang")
    s, L, D = c.s, lib(), c.D
    tau = torch.zeros(N, 6 + D, device="cuda:0")
    eff = torch.zeros(N, D, device="cuda:0")

    def call(sim=s.handle, terms=3, accel=None, out=tau.data_ptr(), efforts=None, dofs=None, num=None):
        arr = None if dofs is None else (C.c_int32 * max(len(dofs), 1))(*dofs)
        n = (0 if dofs is None else len(dofs)) if num is None else num
        rc = L.tg_inverse_dynamics(sim, terms, accel, out, efforts, arr, n, 0)
        return rc, L.tg_last_error()

    assert call()[0] == 0
    assert call(terms=0, accel=c.accel_t.data_ptr())[0] == 0                # no terms, but an accel
    eff_ok = torch.zeros(N, D, device="cuda:0")
    assert call(out=None, efforts=eff_ok.data_ptr(), dofs=[0, D - 1])[0] == 0
    bad = {
        "null sim": dict(sim=None),
        "terms 4": dict(terms=4),
        "terms negative": dict(terms=-1),
        "no terms, no accel": dict(terms=0),
        "no output": dict(out=None),
        "num_dofs negative": dict(dofs=[0], num=-1),
        "num_dofs D + 1": dict(dofs=list(range(D)) + [0], efforts=eff.data_ptr()),
        "null dofs": dict(num=2, efforts=eff.data_ptr()),
        "dof == D": dict(dofs=[0, D], efforts=eff.data_ptr()),
        "negative dof": dict(dofs=[-1], efforts=eff.data_ptr()),
        "dof twice": dict(dofs=[1, 2, 1], efforts=eff.data_ptr()),
        "dof twice, no efforts": dict(dofs=[3, 3]),
    }
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == -1, (what, rc)                                        # TG_ERR_ARG
        assert msg.startswith(b"tg_inverse_dynamics:"), (what, msg)
    torch.cuda.synchronize()
    assert (eff == 0).all()                                                # (a rejected call launches nothing)
    assert (eff_ok[:, 1:D - 1] == 0).all() and (eff_ok[:, [0, D - 1]] != 0).any()


def test_python_argument_checks():
    c = shared("thormang")
    s, D = c.s, c.D
    ok = torch.zeros(N, 6 + D, device="cuda:0")
    with pytest.raises(ValueError):
        s.inverse_dynamics(accel=ok[:, :-1])                                # shape (and contiguity)
    with pytest.raises(ValueError):
        s.inverse_dynamics(accel=ok.double())                               # dtype
    with pytest.raises(ValueError):
        s.inverse_dynamics(accel=ok.cpu())                                  # device
    with pytest.raises(ValueError):
        s.inverse_dynamics(accel=torch.zeros(6 + D, N, device="cuda:0").t())   # contiguity
    with pytest.raises(ValueError):
        s.inverse_dynamics(out=torch.zeros(N, D, device="cuda:0"))
    with pytest.raises(ValueError):
        s.inverse_dynamics(efforts=ok)
    with pytest.raises(ValueError):
        s.inverse_dynamics(efforts=torch.zeros(N, D, device="cuda:0").double())
    with pytest.raises(ValueError):
        s.inverse_dynamics(gravity=False, velocity=False)                   # nothing to compute
    with pytest.raises(ValueError):
        s.inverse_dynamics(dofs=[])
    with pytest.raises(KeyError):
        s.inverse_dynamics(dofs=["no_such_dof"])
    with pytest.raises(RuntimeError, match="tg_inverse_dynamics: DOF"):
        s.inverse_dynamics(dofs=[0, 0])
    with pytest.raises(RuntimeError, match="tg_inverse_dynamics: DOF"):
        s.inverse_dynamics(dofs=[D])
    torch.cuda.synchronize()


def _closed_loop_sim(coasting):
    from thormang_isaacgym_amd.sim import Sim, load_model
    m = load_model("thormang")
    desc, sp, root, dof, props, pt, vt = closed_loop_case(m, coasting=coasting)
    s = Sim(m, sp, CLOSED_LOOP_N, "cuda:0")
    s.root_state.copy_(torch.from_numpy(root))
    s.dof_state.copy_(torch.from_numpy(dof))
    s.dof_props.copy_(torch.from_numpy(props))
    s.dof_pos_target.copy_(torch.from_numpy(pt))
    s.dof_actuation.zero_()
    s.refresh()
    return s, dof


def test_closed_loop_holds_a_posture_on_the_device():
    """The CPU test's held posture (tests/test_id_reference.py): 60 steps of
    inverse_dynamics(efforts=dof_actuation) then simulate hold the posture to
    1e-3 rad under gravity; with zero efforts the robot moves by more than 0.1 rad."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    s, dof0 = _closed_loop_sim(False)
    for _ in range(CLOSED_LOOP_STEPS):
        s.inverse_dynamics(efforts=s.dof_actuation)
        s.simulate()
    torch.cuda.synchronize()
    held = s.dof_state.cpu().numpy().reshape(-1, 2)
    f, _ = _closed_loop_sim(False)
    for _ in range(CLOSED_LOOP_STEPS):
        f.simulate()
    torch.cuda.synchronize()
    free = f.dof_state.cpu().numpy().reshape(-1, 2)
    fig = {"held": float(np.abs(held[:, 0] - dof0[:, 0]).max()), "free": float(np.abs(free[:, 0] - dof0[:, 0]).max())}
    print(fig)
    assert np.isfinite(held).all()
    assert fig["held"] <= HOLD_BOUND and fig["free"] > 0.1, fig


def test_coasting_matches_the_recorded_fp64_loop():
    """The arms moving, both terms on: the device's final joint state is within
    1e-3 of the fp64 reference loop's (reference torques, oracle step), and the
    joint velocities have coasted."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    ref, ref0 = reference_loop("coast")
    s, dof0 = _closed_loop_sim(True)
    assert np.array_equal(dof0, ref0)
    for _ in range(CLOSED_LOOP_STEPS):
        s.inverse_dynamics(efforts=s.dof_actuation)
        s.simulate()
    torch.cuda.synchronize()
    got = s.dof_state.cpu().numpy().reshape(-1, 2)
    fig = {"vs_fp64_loop": float(np.abs(got - ref).max()), "coast_drift": float(np.abs(got[:, 1] - dof0[:, 1]).max()),
           "moved": float(np.abs(got[:, 0] - dof0[:, 0]).max())}
    print(fig)
    assert fig["vs_fp64_loop"] <= 1e-3 and fig["coast_drift"] <= COAST_BOUND, fig
    assert fig["moved"] > 0.1


@pytest.mark.parametrize("link_name,nd,seed", CLOSED_LOOP_CASES)
def test_osc_under_gravity(link_name, nd, seed):
    """The closed-loop setup of tests/test_gpu_osc.py with the sim's gravity at
    -9.81: solve_osc(efforts=dof_actuation), inverse_dynamics(dofs=chain DOFs,
    efforts=dof_actuation, accumulate=True), simulate, 120 steps, meets that
    test's condition (both error norms <= 10 % of their initial value in every
    env).  The control run without the second call ends with a larger position
    error."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from thormang_isaacgym_amd.sim import Sim, load_model
    m = load_model("thormang")
    n, D = 3, m.num_dof
    (desc, sp, root, dof, props, pt, vt), chain, gp, gq = osc_closed_loop_case(m, link_name, nd, seed, n)
    p0, o0 = error_norms(pose_error(m, root, dof, chain, gp, gq))
    gp_t, gq_t = torch.from_numpy(gp[:, None].copy()).cuda(), torch.from_numpy(gq[:, None].copy()).cuda()
    rest_t = torch.from_numpy(dof.reshape(n, D, 2)[:, :, 0].copy()).cuda()
    final = {}
    for compensate in (True, False):
        s = Sim(m, sp, n, "cuda:0")
        s.set_gravity(GRAVITY)
        s.root_state.copy_(torch.from_numpy(root))
        s.dof_state.copy_(torch.from_numpy(dof))
        s.dof_props.copy_(torch.from_numpy(props))
        s.dof_pos_target.copy_(torch.from_numpy(pt))
        s.refresh()
        ch = s.ik_chain(link_name, num_dofs=nd)
        dofs = chain_spec(ch)[1]
        assert list(dofs) == list(chain[1])
        for _ in range(OSC_STEPS):
            s.solve_osc([ch], gp_t, gq_t, q_rest=rest_t, kp=KP, kp_null=KP_NULL, damping=CLOSED_LOOP_DAMPING,
                        efforts=s.dof_actuation)
            if compensate:
                s.inverse_dynamics(dofs=dofs, efforts=s.dof_actuation, accumulate=True)
            s.simulate()
        torch.cuda.synchronize()
        final[compensate] = s.dof_state.cpu().numpy().reshape(-1, 2)
        assert np.isfinite(final[compensate]).all()
    p1, o1 = error_norms(pose_error(m, root, final[True], chain, gp, gq))
    pc, oc = error_norms(pose_error(m, root, final[False], chain, gp, gq))
    print({"link": link_name, "pos": (float(p0.max()), float(p1.max())), "orn": (float(o0.max()), float(o1.max())),
           "worst_ratio": (float((p1 / p0).max()), float((o1 / o0).max())),
           "without_compensation": {"pos": float(pc.max()), "orn": float(oc.max()),
                                    "worst_ratio": (float((pc / p0).max()), float((oc / o0).max()))}})
    assert (p1 <= 0.10 * p0).all() and (o1 <= 0.10 * o0).all(), (p0, p1, o0, o1)
    assert (pc > p1).all(), (pc, p1)
