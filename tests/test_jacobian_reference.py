"""The float64 reference of the Jacobian and mass-matrix tensors
(tests/jacobian_ref.py) means what include/tgsim.h says: J u gives the oracle's
link velocities, the oracle's physics step accelerates as H says, and a
pendulum's H is the textbook one.  No GPU needed; the kernels are held to this
reference in tests/test_gpu_jacobian.py."""
import numpy as np
import pytest

from tests import physics_models as pm
from tests.jacobian_ref import jacobian_ref, mass_matrix_ref
from tests.oracle_lib import physics_step, rigid_body_states
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.sim import load_model


def _model(name):
    return pm.chain() if name == "kat_chain" else load_model(name)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_reference_jacobian_times_u_is_the_oracle_link_velocity(name):
    m = load_model(name)
    desc = abi.ModelDesc(m)
    n, D = 3, m.num_dof
    root, dof = random_state(m, n, np.random.default_rng(11))
    J = jacobian_ref(m, root, dof, desc)
    u = np.concatenate([root[:, 7:13], dof.reshape(n, D, 2)[:, :, 1]], axis=1).astype(np.float64)
    v = rigid_body_states(desc, root, dof)[..., 7:13]
    err = float(np.abs(np.einsum("nlrc,nc->nlr", J, u) - v).max())
    print({"model": name, "max_abs_J": float(np.abs(J).max()), "J_u_vs_oracle": err})
    assert err <= 1e-6, err


@pytest.mark.parametrize("name", ["kat_chain", "thormang", "gogoro"])
def test_oracle_step_accelerates_as_the_reference_mass_matrix_says(name):
    """Zero gravity, from rest, effort mode without limits: one oracle step of
    dt gives velocities / dt = solve(H[idx, idx], (0_6, tau)[idx]), idx the base
    plus the free DOFs -- the step's dynamics are those of H with the locked
    rows and columns removed."""
    m = _model(name)
    D = m.num_dof
    dt = 0.001
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=1, dt=dt, substeps=1, gravity=(0, 0, 0))
    root[0, 2] = 10.0
    lo, hi = props[abi.TG_PROP_LOWER, 0], props[abi.TG_PROP_UPPER, 0]
    limited = (np.abs(lo) < 1e30) & (np.abs(hi) < 1e30)
    dof[:, 0] = np.where(limited, 0.5 * (lo.astype(np.float64) + hi), 0.0)
    props[abi.TG_PROP_DRIVE_MODE] = 3
    props[abi.TG_PROP_EFFORT] = 1e30
    props[abi.TG_PROP_VELOCITY] = 1e30
    props[abi.TG_PROP_STIFFNESS] = 0.0
    props[abi.TG_PROP_DAMPING] = 0.0
    locked = np.zeros(D, bool)
    locked[list(m.locked_dofs)] = True
    rs = np.random.default_rng(7)
    tau = np.where(locked, 0.0, rs.uniform(-1.0, 1.0, D)).astype(np.float32).reshape(1, D)
    H = mass_matrix_ref(m, root, dof, armature=props[abi.TG_PROP_ARMATURE], desc=desc)[0]
    idx = np.concatenate([np.arange(6), 6 + np.flatnonzero(~locked)])
    rhs = np.concatenate([np.zeros(6), tau[0].astype(np.float64)])[idx]
    acc_ref = np.linalg.solve(H[np.ix_(idx, idx)], rhs)
    physics_step(desc, sp, root, dof, props, pt, vt, act=tau)
    acc = np.concatenate([root[0, 7:13], dof[:, 1]]).astype(np.float64)[idx] / dt
    err, scale = float(np.abs(acc - acc_ref).max()), float(np.abs(acc_ref).max())
    print({"model": name, "locked": int(locked.sum()), "rel_err": err / scale})
    assert err <= 1e-5 * scale, (err, scale)


def test_pendulum_mass_matrix_known_answer():
    """H[6, 6] of a pendulum of length l: Ic + m l^2 + armature."""
    l, mass, Ic, arm = 0.5, 1.3, 0.02, 0.04
    m = pm.pendulum(l=l, mass=mass, Ic=Ic)
    root = np.zeros((1, 13), np.float32)
    root[0, 6] = 1.0
    dof = np.array([[0.6, 0.0]], np.float32)
    H = mass_matrix_ref(m, root, dof, armature=np.array([[arm]]))
    expect = float(np.float32(Ic)) + float(np.float32(mass)) * float(np.float32(l)) ** 2 + arm
    assert abs(H[0, 6, 6] - expect) <= 1e-6 * expect, (H[0, 6, 6], expect)
