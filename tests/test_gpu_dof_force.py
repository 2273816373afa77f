"""DOF force tensor (tg_set_dof_force_tensor) on the GPU.

* pendulums: the inverse-dynamics identity (I + armature) dqd / h - tau_g =
  out, which knows nothing of the PD law;
* chain, gogoro and thormang (the latter two standing on the ground): out =
  te - K (qd1 - qd0) / h from the GPU's own before / after state, and against
  the fp64 oracle with the oracle's fp32 build as the yardstick;
* saturation on each clamp path (Woodbury, its fallback, the rerun): +-effort
  bit-exactly; the mean over substeps; a full rewrite by every simulate;
* nothing else moves: the physics is bit-identical with and without the
  tensor, the contact tensor is unchanged beside it, and the walk task's obs /
  reward / resets do not depend on it.

Batches are ragged against the workgroup (35 envs: three workgroups of 16)
with a different state per env.  Every bound is derived from the float32
rounding of the states the formula is evaluated on (see ``pd_bound``)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.oracle_lib import lib as oracle_lib, physics_step
from thormang_isaacgym_amd.abi import (TG_PROP_ARMATURE, TG_PROP_DAMPING, TG_PROP_DRIVE_MODE, TG_PROP_EFFORT,
                                       TG_PROP_STIFFNESS, TG_PROP_VELOCITY)

pytestmark = pytest.mark.gpu

N = 35
POS, VEL, EFFORT = 1, 2, 3
TG_ERR_MODEL = -3


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def _sp(sp, **kw):
    c = type(sp).from_buffer_copy(sp)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _h(sp):
    """The substep as the library forms it (float32 dt / substeps)."""
    return float(np.float32(sp.dt) / np.float32(sp.substeps))


# ------------------------------------------------------------------ states (CPU, cached, never modified)
_ST = {}


def _unlocked(desc):
    return np.nonzero(np.asarray(desc.arrays["dof_locked"]) == 0)[0]


def _state(name):
    """Start states: dict(m, desc, sp, root [N,13], dof [N*D,2], props [P,N,D],
    pt, vt [N,D]), efforts 1e30, a different state per env.  thormang / gogoro:
    the contact-force test's standing starts (reset pose, random yaw and tilt,
    the lowest shape point 0..1 mm inside the ground) with random joint
    velocities and target offsets on the free DOFs; kat_chain: a spinning free
    chain, POS drive on the revolute DOF and VEL drive on the prismatic one."""
    if name in _ST:
        return _ST[name]
    rs = np.random.default_rng(21)
    if name in ("thormang", "gogoro", "thormang_wb"):
        from tests.test_gpu_contact_force import _articulated_state
        a = _articulated_state(name)
        m, desc, sp = a["m"], a["o"].desc, a["o"].sp
        root, dof, props, pt, vt = (a[k].copy() for k in ("root", "dof", "props", "pt", "vt"))
        D, free = m.num_dof, _unlocked(desc)
        dof.reshape(N, D, 2)[:, free, 1] = rs.normal(0, 0.3, (N, len(free)))
        pt[:, free] += rs.normal(0, 0.05, (N, len(free))).astype(np.float32)
        if name == "gogoro":   # a drive on every free DOF: POS, VEL (as the task's rear wheel), and the grips
            for k, d in enumerate(free):
                if props[TG_PROP_DRIVE_MODE, 0, d] == 0:
                    props[TG_PROP_DRIVE_MODE, :, d] = POS
                    props[TG_PROP_STIFFNESS, :, d] = 40.0 + 10 * k
                    props[TG_PROP_DAMPING, :, d] = 2.0 + k
            vt[:, free] += rs.normal(0, 0.5, (N, len(free))).astype(np.float32)
    else:
        assert name == "kat_chain"
        m = pm.chain()
        desc, sp, root, dof, props, pt, vt = pm.sim(m, n=N, dt=0.005, substeps=1)
        root[:, 2] = 1.0
        root[:, 7:10] = rs.normal(0, 1, (N, 3))
        root[:, 10:13] = rs.normal(0, 2, (N, 3))
        dof[:, 0] = rs.uniform(-0.5, 0.5, 2 * N)
        dof[:, 1] = rs.normal(0, 1, 2 * N)
        props[TG_PROP_DRIVE_MODE, :, 0], props[TG_PROP_DRIVE_MODE, :, 1] = POS, VEL
        props[TG_PROP_STIFFNESS, :, 0], props[TG_PROP_DAMPING, :, 0] = 60.0, 4.0
        props[TG_PROP_STIFFNESS, :, 1], props[TG_PROP_DAMPING, :, 1] = 0.0, 30.0
        props[TG_PROP_ARMATURE] = 0.01
        pt[:] = rs.uniform(-0.5, 0.5, (N, 2))
        vt[:] = rs.uniform(-1, 1, (N, 2))
    props[TG_PROP_EFFORT] = 1e30
    _ST[name] = dict(m=m, desc=desc, sp=sp, root=root, dof=dof, props=props, pt=pt, vt=vt)
    return _ST[name]


def _with(st, **kw):
    return dict(st, **kw)


# ------------------------------------------------------------------ running
def _sim(st, sp, act=None, contact=False, dof_force=True, hf=False):
    from thormang_isaacgym_amd.sim import Sim
    s = Sim(st["m"], sp, N, "cuda:0")
    assert not s.jit
    s.root_state.copy_(torch.from_numpy(st["root"]))
    s.dof_state.copy_(torch.from_numpy(st["dof"]))
    s.dof_props.copy_(torch.from_numpy(st["props"]))
    s.dof_pos_target.copy_(torch.from_numpy(st["pt"]))
    s.dof_vel_target.copy_(torch.from_numpy(st["vt"]))
    if act is not None:
        s.dof_actuation.copy_(torch.from_numpy(act))
        s.set_dof_actuation_forces(s.dof_actuation)
    s.env_dirty.fill_(1)
    if hf:   # a level terrain under every env: the heightfield instantiation of the step kernel
        s.set_heightfield(np.zeros((100, 100), np.float32), 0.5, 1.0, -10.0, -10.0, friction=float(sp.ground_friction))
    cf = s.acquire_net_contact_force_tensor() if contact else None
    df = s.acquire_dof_force_tensor() if dof_force else None
    return s, df, cf


def _gpu_step(st, sp, act=None, calls=1, hf=False):
    """``calls`` simulates from the start state: per call the tensor and the
    dof state after it ([N,D] float64, [N,D,2] float32)."""
    s, df, _ = _sim(st, sp, act, hf=hf)
    D = st["m"].num_dof
    assert df.shape == (N, D) and df is s.acquire_dof_force_tensor()
    out = []
    for _ in range(calls):
        s.simulate()
        out.append((df.cpu().numpy().astype(np.float64), s.dof_state.cpu().numpy().reshape(N, D, 2).copy(),
                    s.root_state.cpu().numpy().copy()))
    s.close()
    return out


def _oracle_step(st, sp, precision, act=None):
    root, dof = st["root"].copy(), st["dof"].copy()
    physics_step(st["desc"], sp, root, dof, st["props"], st["pt"].copy(), st["vt"].copy(), act=act, threads=4,
                 L=oracle_lib(precision))
    return dof.reshape(N, st["m"].num_dof, 2)


# ------------------------------------------------------------------ the law and its bound
def pd_law(st, dof0, dof1, h):
    """te - K (qd1 - qd0) / h per drive DOF in float64 from float32 states, 0 elsewhere."""
    p = st["props"].astype(np.float64)
    kp, kd, mode = p[TG_PROP_STIFFNESS], p[TG_PROP_DAMPING], np.rint(p[TG_PROP_DRIVE_MODE])
    d0, d1 = dof0.astype(np.float64), dof1.astype(np.float64)
    q0, qd0, qd1 = d0[..., 0], d0[..., 1], d1[..., 1]
    te = kp * (st["pt"].astype(np.float64) - q0 - h * qd0) + kd * (st["vt"].astype(np.float64) - qd0)
    K = h * kd + h * h * kp
    return np.where((mode == POS) | (mode == VEL), te - K * (qd1 - qd0) / h, 0.0)


C_PD = 8


def pd_bound(st, dof0, dof1, h, tau):
    """C_PD (kp (ulp32(q) + h ulp32(qd)) + (kd + h kp) ulp32(qd)) + 1e-5 |tau|,
    q the largest of |q0|, |q*| and qd the largest of |qd0|, |qd1|, |qd*|.
    The kernel evaluates the same formula in float32 on the same states, so
    the difference is rounding alone: the differences q* - q0 and qd* - qd0,
    the product h qd0, the sum inside te and qd1 - qd0 each round to half an
    ulp of their largest operand (3 such in the kp term, 2 at the (kd + h kp)
    scale), the gain products and K add 2^-24 of their results (below one more
    ulp of the operands each, 2^-24 |x| <= ulp32(x)), and 1 / h is the
    hardware reciprocal, one ulp on K dqd / h.  That is under 4 ulp per term;
    C_PD = 8 leaves a factor of 2.  Undriven DOFs: 0, exactly."""
    p = st["props"].astype(np.float64)
    kp, kd, mode = p[TG_PROP_STIFFNESS], p[TG_PROP_DAMPING], np.rint(p[TG_PROP_DRIVE_MODE])
    q = np.maximum(np.abs(dof0[..., 0]), np.abs(st["pt"]))
    qd = np.maximum(np.maximum(np.abs(dof0[..., 1]), np.abs(dof1[..., 1])), np.abs(st["vt"]))
    b = C_PD * (kp * (ulp32(q) + h * ulp32(qd)) + (kd + h * kp) * ulp32(qd)) + 1e-5 * np.abs(tau)
    return np.where((mode == POS) | (mode == VEL), b, 0.0)


def _check_law(what, st, sp, out, dof1, skip=None):
    h = _h(sp)
    dof0 = st["dof"].reshape(N, -1, 2)
    tau = pd_law(st, dof0, dof1, h)
    b = pd_bound(st, dof0, dof1, h, tau)
    err = np.abs(out - tau)
    if skip is not None:
        err, b = np.where(skip, 0.0, err), np.where(skip, 1.0, b)
    drv = b > 0
    print(what, "PD law: max |tau| %.3e, max err %.3e, min bound %.3e, worst err/bound %.3f over %d entries"
          % (np.abs(tau).max(), err.max(), b[drv].min() if drv.any() else 0.0,
             (err[drv] / b[drv]).max() if drv.any() else 0.0, int(drv.sum())))
    assert np.isfinite(out).all()
    assert (err <= b).all(), (what, float(err.max()), np.argwhere(err > b)[:5].tolist())
    return tau


# ------------------------------------------------------------------ 1. inverse dynamics
C_ID = 16


@pytest.mark.parametrize("axis", ["y", "z"])
@pytest.mark.parametrize("mode", [POS, VEL, EFFORT])
def test_pendulum_inverse_dynamics_identity(axis, mode):
    """kat_pendulum_y / _z, fixed base, one substep, gravity on: (I_axis +
    armature) (qd1 - qd0) / h - tau_g(q0) = out per env, tau_g = -m g l sin q0
    about y and 0 about z; the right side never sees the drive law.  POS and
    VEL drives with random state and targets, effort 1e30; EFFORT mode with
    random actuation, a third of it beyond the effort (the clamp).

    I_axis = Ic + m l^2 about y; about z the arm's centre of mass lies on the
    axis and I_axis = Ic.

    Bound: C_ID ulp32(max |qd|) I / h + 1e-5 |tau|, I = I_axis + armature,
    C_ID = 16, speeds drawn with |qd0| in [1, 3] rad/s so that one ulp of qd is
    at least 1.2e-7.  Why 16: the stored qd1 is rounded to half an ulp, which
    moves the left side by I / (2 h) and the implicit law by K / (2 h) <= I /
    (2 h) for the gains used (kd + h kp <= 12 about y, where I / h = 26, and
    <= 0.48 about z, where I / h >= 1): 1 ulp I / h.  The
    kernel's acceleration comes from a float32 solve of (I + K) qdd = te - tau_g
    - ...: four roundings at the scale of the torques, worth below 2 ulp I / h
    at these speeds (2^-24 x 50 N m = 3e-6 = 1 ulp I / h at |qd| = 1), and the
    hardware sine of the joint angle (absolute error about 1e-6) moves tau_g =
    4.9 sin q0 by up to 5e-6, another 2 ulp I / h.  About 7 in all; 16 leaves a
    factor of 2."""
    _cuda()
    l, mass, Ic = 0.5, 1.0, float(np.float32(0.01))
    m = pm.pendulum(axis="0 1 0" if axis == "y" else "0 0 1")
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=N, dt=0.01, substeps=1, fix_base_link=True)
    rs = np.random.default_rng(100 + 10 * mode + (axis == "z"))
    props[TG_PROP_DRIVE_MODE] = mode
    props[TG_PROP_ARMATURE, :, 0] = rs.uniform(0.0, 0.05, N)
    props[TG_PROP_VELOCITY] = 0.0
    dof[:, 0] = rs.uniform(-1.5, 1.5, N)
    dof[:, 1] = rs.uniform(1.0, 3.0, N) * rs.choice([-1.0, 1.0], N)
    act = None
    if mode == EFFORT:
        props[TG_PROP_EFFORT] = 5.0
        act = rs.uniform(-7.5, 7.5, (N, 1)).astype(np.float32)
        assert (np.abs(act) > 5.0).sum() >= 5
    else:
        props[TG_PROP_EFFORT] = 1e30
        gs = 1.0 if axis == "y" else 0.04   # (gains in proportion to the inertia about the axis)
        props[TG_PROP_STIFFNESS, :, 0] = gs * rs.uniform(20, 200, N)
        props[TG_PROP_DAMPING, :, 0] = gs * rs.uniform(1, 10, N)
        pt[:, 0] = rs.uniform(-1, 1, N)
        vt[:, 0] = rs.uniform(-1, 1, N)
    st = dict(m=m, desc=desc, sp=sp, root=root, dof=dof, props=props, pt=pt, vt=vt)
    (out, dof1, _), = _gpu_step(st, sp, act)
    h, g = _h(sp), -float(sp.gravity[2])
    q0, qd0, qd1 = (x.astype(np.float64) for x in (dof[:, 0], dof[:, 1], dof1[:, 0, 1]))
    inertia = Ic + (mass * l * l if axis == "y" else 0.0) + props[TG_PROP_ARMATURE, :, 0].astype(np.float64)
    tau_g = -mass * g * l * np.sin(q0) if axis == "y" else 0.0
    want = inertia * (qd1 - qd0) / h - tau_g
    err = np.abs(out[:, 0] - want)
    bound = C_ID * ulp32(np.maximum(np.abs(qd0), np.abs(qd1))) * inertia / h + 1e-5 * np.abs(want)
    print("pendulum", axis, "mode", mode, "max |tau| %.3e, max err %.3e, min bound %.3e, worst err/bound %.3f"
          % (np.abs(want).max(), err.max(), bound.min(), (err / bound).max()))
    free = np.ones(N, bool) if act is None else np.abs(act[:, 0]) < 5.0   # (clamped actuations repeat +-5)
    assert len({float(x) for x in out[free, 0]}) == int(free.sum()), "every env has its own value"
    assert (err <= bound).all(), (float(err.max()), float((err / bound).max()))
    if mode == EFFORT:   # and the value itself: the clamped actuation, exactly
        assert np.array_equal(out[:, 0].astype(np.float32), np.clip(act[:, 0], -5.0, 5.0))
    else:
        _check_law("pendulum_%s mode %d" % (axis, mode), st, sp, out, dof1)


def test_effort_mode_with_zero_actuation_reads_zero():
    _cuda()
    m = pm.pendulum()
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=N, dt=0.01, substeps=1, fix_base_link=True)
    props[TG_PROP_DRIVE_MODE] = EFFORT
    props[TG_PROP_EFFORT] = 5.0
    dof[:, 0] = np.linspace(-1, 1, N)
    (out, dof1, _), = _gpu_step(dict(m=m, desc=desc, sp=sp, root=root, dof=dof, props=props, pt=pt, vt=vt), sp)
    assert (out == 0).all() and np.abs(dof1[:, 0, 1]).max() > 0


# ------------------------------------------------------------------ 2. the law on the GPU's own states
@pytest.mark.parametrize("solver", [1, 0])
@pytest.mark.parametrize("name", ["kat_chain", "gogoro", "thormang"])
def test_pd_law_on_the_gpus_own_states(name, solver):
    """out = te - K (qd1 - qd0) / h, float64 from the float32 states before and
    after one substep (TGS and PGS; gogoro and thormang with live contacts, so
    qd1 includes the contact impulses), within ``pd_bound``; locked DOFs read
    exactly 0."""
    _cuda()
    st = _state(name)
    sp = _sp(st["sp"], substeps=1, solver_type=solver)
    (out, dof1, root1), = _gpu_step(st, sp)
    assert np.isfinite(root1).all()
    tau = _check_law("%s solver %d" % (name, solver), st, sp, out, dof1)
    locked = np.nonzero(np.asarray(st["desc"].arrays["dof_locked"]) != 0)[0]
    assert (out[:, locked] == 0).all()
    if name == "gogoro":
        assert len(locked) > 0
    free = _unlocked(st["desc"])
    assert len({tuple(out[e, free]) for e in range(N)}) == N, "every env has its own values"
    assert (np.abs(tau[:, free]).max(axis=0) > 0).all(), "every free DOF is driven in this test"


@pytest.mark.parametrize("name,hf", [("gogoro", True), ("thormang", True), ("thormang_wb", False)])
def test_pd_law_on_terrain_and_on_the_whole_body_model(name, hf):
    """The kernel's other instantiations: the heightfield ones (a level
    terrain, so the same contacts) and the whole-body humanoid's (8 envs per
    workgroup: 35 envs are five workgroups, the last one ragged)."""
    _cuda()
    st = _state(name)
    sp = _sp(st["sp"], substeps=1)
    (out, dof1, root1), = _gpu_step(st, sp, hf=hf)
    assert np.isfinite(root1).all()
    tau = _check_law("%s%s" % (name, " on a heightfield" if hf else ""), st, sp, out, dof1)
    free = _unlocked(st["desc"])
    assert (np.abs(tau[:, free]).max(axis=0) > 0).all()
    assert len({tuple(out[e, free]) for e in range(N)}) == N


# ------------------------------------------------------------------ 3. against the fp64 oracle
@pytest.mark.parametrize("name", ["kat_chain", "gogoro", "thormang"])
def test_matches_the_fp64_oracle(name):
    """The same starts stepped by the fp64 oracle (one substep, TGS): tau_ref
    is the law on the oracle's states; the yardstick is the oracle's own fp32
    build through the same formula.  The GPU's largest error over all 35 envs
    may be at most 4x the yardstick's (the contact-force test's ratio).
    Measured on the MI355X, GPU / control: kat_chain 8.3e-6 /
    8.2e-6 (ratio 1.02), gogoro 1.03e-4 / 9.2e-5 N m (1.12), thormang 6.5e-4 /
    4.3e-4 N m (1.51)."""
    _cuda()
    st = _state(name)
    sp = _sp(st["sp"], substeps=1, solver_type=1)
    h = _h(sp)
    dof0 = st["dof"].reshape(N, -1, 2)
    (out, dof1, _), = _gpu_step(st, sp)
    ref = pd_law(st, dof0, _oracle_step(st, sp, "f64"), h)
    ctl = pd_law(st, dof0, _oracle_step(st, sp, "f32"), h)
    e_gpu, e_ctl = np.abs(out - ref).max(axis=1), np.abs(ctl - ref).max(axis=1)
    print(name, "tau error vs fp64 oracle over all envs: GPU %.4e, fp32 oracle (control) %.4e, ratio %.2f; "
          "median env GPU %.4e, control %.4e; max |tau| %.3e"
          % (e_gpu.max(), e_ctl.max(), e_gpu.max() / max(e_ctl.max(), 1e-300), np.median(e_gpu), np.median(e_ctl),
             np.abs(ref).max()))
    assert e_gpu.max() <= 4 * e_ctl.max(), (e_gpu.max(), e_ctl.max())


# ------------------------------------------------------------------ 4. saturation
def _lifted(st, dz=1.0):
    root = st["root"].copy()
    root[:, 2] += dz
    return _with(st, root=root)


def _saturation_case(st, sp, pick):
    """Efforts chosen from the CPU oracle's states so that the margins are a
    factor of 4: the oracle (fp64) steps the start with every effort 1e30 and
    no velocity limit, out of contact, so ti = te - K (qd1 - qd0) / h is the
    first solve's implicit torque; drive DOFs in ``pick`` get effort |ti| / 4,
    the other drives 4 |ti| + 1.  Returns the state with those efforts, the
    saturated mask and sign(ti)."""
    props = st["props"].copy()
    props[TG_PROP_EFFORT] = 1e30
    props[TG_PROP_VELOCITY] = 0.0
    st = _with(st, props=props)
    h = _h(sp)
    dof0 = st["dof"].reshape(N, -1, 2)
    ti = pd_law(st, dof0, _oracle_step(st, sp, "f64"), h)
    mode = np.rint(props[TG_PROP_DRIVE_MODE])
    drv = (mode == POS) | (mode == VEL)
    sat = np.zeros_like(drv)
    sat[:, pick] = True
    sat &= drv
    eff = np.where(sat, np.abs(ti) / 4, 4 * np.abs(ti) + 1).astype(np.float32)
    props = props.copy()
    props[TG_PROP_EFFORT] = np.where(drv, eff, props[TG_PROP_EFFORT])
    # the intended sides, on the oracle's states: saturated at least 2x beyond, the rest at most 0.5x
    e64 = props[TG_PROP_EFFORT].astype(np.float64)
    assert (np.abs(ti)[sat] >= 2 * e64[sat]).all() and (e64[sat] > 0).all()
    assert (np.abs(ti)[drv & ~sat] <= 0.5 * e64[drv & ~sat]).all()
    return _with(st, props=props), sat, np.sign(ti)


def _check_saturated(what, st, sp, sat, sgn):
    (out, dof1, _), = _gpu_step(st, sp)
    eff = st["props"][TG_PROP_EFFORT]
    want = (sgn * eff).astype(np.float32)
    got = out.astype(np.float32)
    print(what, "saturated entries per env: %d..%d" % (sat.sum(axis=1).min(), sat.sum(axis=1).max()),
          "bit-exact:", bool(np.array_equal(got[sat].view(np.uint32), want[sat].view(np.uint32))))
    assert np.array_equal(got[sat].view(np.uint32), want[sat].view(np.uint32)), \
        np.abs(got[sat] - want[sat]).max()
    _check_law(what + " (unsaturated drives)", st, sp, out, dof1, skip=sat)


def test_saturation_woodbury_pendulum():
    """|ti| >> effort on a pendulum (one clamped drive: the Woodbury update)."""
    _cuda()
    m = pm.pendulum()
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=N, dt=0.01, substeps=1, fix_base_link=True)
    rs = np.random.default_rng(5)
    props[TG_PROP_DRIVE_MODE] = POS
    props[TG_PROP_STIFFNESS, :, 0] = rs.uniform(100, 400, N)
    props[TG_PROP_DAMPING, :, 0] = rs.uniform(2, 10, N)
    dof[:, 0] = rs.uniform(-1, 1, N)
    dof[:, 1] = rs.uniform(-1, 1, N)
    pt[:, 0] = dof[:, 0] + rs.uniform(1.0, 2.0, N) * rs.choice([-1.0, 1.0], N)
    st, sat, sgn = _saturation_case(dict(m=m, desc=desc, sp=sp, root=root, dof=dof, props=props, pt=pt, vt=vt), sp, [0])
    assert sat.all() and (sgn > 0).any() and (sgn < 0).any()
    _check_saturated("pendulum (Woodbury)", st, sp, sat, sgn)


@pytest.mark.parametrize("nsat", [2, 3, 4])
def test_saturation_gogoro_woodbury_and_fallback(nsat):
    """gogoro in the air, a drive on each of its 5 free DOFs: exactly 2
    saturated (the Woodbury update), 3 and 4 (more than it takes: the rerun)."""
    _cuda()
    st0 = _lifted(_state("gogoro"))
    sp = _sp(st0["sp"], substeps=1)
    free = _unlocked(st0["desc"])
    pt = st0["pt"].copy()
    rs = np.random.default_rng(6)
    pt[:, free] += (rs.uniform(0.3, 0.6, (N, len(free))) * rs.choice([-1.0, 1.0], (N, len(free)))).astype(np.float32)
    st, sat, sgn = _saturation_case(_with(st0, pt=pt), sp, list(free[:nsat]))
    assert (sat.sum(axis=1) == nsat).all()
    _check_saturated("gogoro, %d saturated" % nsat, st, sp, sat, sgn)


def test_saturation_thormang_rerun():
    """thormang with a fixed base, in the air (NG > 8: the plain rerun): every
    third free DOF far beyond a small effort, the rest far below theirs."""
    _cuda()
    st0 = _lifted(_state("thormang"))
    sp = _sp(st0["sp"], substeps=1, fix_base=1)
    free = _unlocked(st0["desc"])
    pick = list(free[::3])
    pt = st0["pt"].copy()
    rs = np.random.default_rng(8)
    pt[:, pick] += (rs.uniform(0.3, 0.6, (N, len(pick))) * rs.choice([-1.0, 1.0], (N, len(pick)))).astype(np.float32)
    st, sat, sgn = _saturation_case(_with(st0, pt=pt), sp, pick)
    assert (sat.sum(axis=1) == len(pick)).all() and len(pick) == 11
    _check_saturated("thormang, 11 of 33 saturated", st, sp, sat, sgn)


# ------------------------------------------------------------------ 5. mean over substeps
@pytest.mark.parametrize("name", ["kat_chain", "thormang"])
def test_mean_over_substeps(name):
    """substeps = 2 over dt against two substeps = 1 calls over dt / 2: the
    tensor is the mean of the two calls', within the mean of their bounds."""
    _cuda()
    st = _state(name)
    sp2 = _sp(st["sp"], substeps=2, solver_type=1)
    sp1 = _sp(st["sp"], substeps=1, solver_type=1, dt=float(np.float32(sp2.dt) / np.float32(2)))
    assert _h(sp1) == _h(sp2)
    (out2, dofe, roote), = _gpu_step(st, sp2)
    (oa, dofa, _), (ob, dofb, rootb) = _gpu_step(st, sp1, calls=2)
    same = np.array_equal(dofe.view(np.uint32), dofb.view(np.uint32)) and \
        np.array_equal(roote.view(np.uint32), rootb.view(np.uint32))
    print(name, "end states of 1 x 2 substeps and 2 x 1 substep bit-identical:", same)
    h = _h(sp1)
    dof0 = st["dof"].reshape(N, -1, 2)
    ta = pd_law(st, dof0, dofa, h)
    stb = _with(st, dof=dofa.reshape(-1, 2))
    tb = pd_law(stb, dofa, dofb, h)
    b = 0.5 * (pd_bound(st, dof0, dofa, h, ta) + pd_bound(stb, dofa, dofb, h, tb))
    err_calls = np.abs(out2 - 0.5 * (oa + ob))
    err_law = np.abs(out2 - 0.5 * (ta + tb))
    drv = b > 0
    print(name, "mean over substeps: vs the two calls max %.3e, vs the law max %.3e, worst / bound %.3f and %.3f"
          % (err_calls.max(), err_law.max(), (err_calls[drv] / b[drv]).max(), (err_law[drv] / b[drv]).max()))
    assert (err_calls <= b).all() and (err_law <= b).all()


# ------------------------------------------------------------------ 6. structure
def test_every_simulate_rewrites_the_tensor_and_null_turns_it_off():
    _cuda()
    from thormang_isaacgym_amd._lib import check, lib
    st = _state("gogoro")
    s, df, _ = _sim(st, st["sp"])
    assert float(df.abs().max()) == 0.0, "zeros until the first simulate"
    df.fill_(float("nan"))
    s.simulate()
    assert bool(torch.isfinite(df).all()), "locked DOFs included"
    assert float(df.abs().max()) > 0
    s.refresh_dof_force_tensor()
    sp = s.get_sim_params()
    sub = sp.substeps
    sp.substeps = 0
    s.set_sim_params(sp)
    df.fill_(float("nan"))
    s.simulate()
    assert float(df.abs().max()) == 0.0
    sp.substeps = sub
    s.set_sim_params(sp)
    check(lib().tg_set_dof_force_tensor(s.handle, None), "disable")
    df.fill_(float("nan"))
    s.simulate()
    assert bool(torch.isnan(df).all())
    s.close()


def test_jit_model_is_refused_with_a_message():
    _cuda()
    from thormang_isaacgym_amd._lib import lib
    from thormang_isaacgym_amd.sim import Sim
    m = pm.jit_walker()
    desc, sp, *_ = pm.sim(m, n=4)
    s = Sim(m, sp, 4, "cuda:0")
    assert s.jit
    t = torch.full((4, s.D), 5.0, device="cuda:0")
    rc = lib().tg_set_dof_force_tensor(s.handle, C.c_void_p(t.data_ptr()))
    assert rc == TG_ERR_MODEL and b"compiled-in" in lib().tg_last_error()
    with pytest.raises(RuntimeError, match="compiled-in"):
        s.acquire_dof_force_tensor()
    s.simulate()
    assert float(t.min()) == 5.0 and float(t.max()) == 5.0
    s.close()


# ------------------------------------------------------------------ 7. nothing else moves
@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_physics_and_contact_tensor_do_not_depend_on_the_tensor(name):
    """20 steps: root and dof state bit-identical with the tensor on and off;
    with both tensors on, the contact tensor matches the contact-only run
    (bit-identical expected; else the contact-force test's own tolerance, 4x
    the fp32 control's error it records, 6.8e-3 N on thormang and 2.8e-4 N on
    gogoro, and the difference printed)."""
    _cuda()
    st = _state(name)

    def run(dof_force, contact):
        s, df, cf = _sim(st, st["sp"], contact=contact, dof_force=dof_force)
        for _ in range(20):
            s.simulate()
        out = (s.root_state.cpu().numpy().copy(), s.dof_state.cpu().numpy().copy(),
               None if cf is None else cf.cpu().numpy().copy(), None if df is None else df.cpu().numpy().copy())
        s.close()
        return out

    r0, d0, _, _ = run(False, False)
    r1, d1, _, f1 = run(True, False)
    r2, d2, c2, _ = run(False, True)
    r3, d3, c3, f3 = run(True, True)
    assert np.isfinite(r0).all() and np.abs(f1).max() > 0 and np.abs(c2).max() > 0
    for r, d in ((r1, d1), (r2, d2), (r3, d3)):
        assert np.array_equal(r0.view(np.uint32), r.view(np.uint32))
        assert np.array_equal(d0.view(np.uint32), d.view(np.uint32))
    assert np.array_equal(f1.view(np.uint32), f3.view(np.uint32))
    same = np.array_equal(c2.view(np.uint32), c3.view(np.uint32))
    print(name, "contact tensor beside the DOF force tensor bit-identical:", same,
          "max difference %.3e N" % np.abs(c2 - c3).max())
    assert same or np.abs(c2 - c3).max() <= 4 * {"thormang": 6.8e-3, "gogoro": 2.8e-4}[name]


def test_walk_task_exposes_dof_forces_and_is_otherwise_unchanged():
    """ThormangWalk with env.enableDofForceSensors against one without, same
    seed, teacher-forced as tests/test_gpu_contact_force.py (the enabled task
    runs the separate post-physics launch; the project's bar for that pair is
    1e-5 per step): resets, time-outs and progress identical, obs and reward
    within 1e-5.  extras["dof_force"] is the sim's tensor."""
    _cuda()
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_cfg
    envs = []
    for on in (False, True):
        cfg = walk_cfg(N)
        if on:
            cfg["env"]["enableDofForceSensors"] = True
        envs.append(make_gpu_walk(cfg, NumpyDraws(5)))
    off, on = envs
    D = on.model.num_dof
    assert off.dof_forces is None and "dof_force" not in off.extras
    assert on.dof_forces.shape == (N, D) and on.dof_forces is on.sim.acquire_dof_force_tensor()
    assert on.acquire_dof_force_tensor() is on.dof_forces
    on.refresh_dof_force_tensor()
    rs = np.random.default_rng(9)
    dobs = drew = seen = 0.0
    for _ in range(20):
        for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "actions", "last_actions", "commands"):
            getattr(on, name).copy_(getattr(off, name))
        on.sim.root_state.copy_(off.sim.root_state)
        on.sim.dof_state.copy_(off.sim.dof_state)
        if off.push_enabled:
            on.sim.body_force.copy_(off.sim.body_force)
        act = torch.from_numpy(rs.uniform(-0.5, 0.5, (N, D)).astype(np.float32)).cuda()
        o0, r0, z0, x0 = off.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        assert torch.equal(z0, z1) and torch.equal(x0["time_outs"], x1["time_outs"])
        assert torch.equal(off.progress_buf, on.progress_buf)
        dobs = max(dobs, float((o0["obs"] - o1["obs"]).abs().max()))
        drew = max(drew, float((r0 - r1).abs().max()))
        f = x1["dof_force"]
        assert f.shape == (N, D) and torch.equal(f, on.sim.acquire_dof_force_tensor())
        assert bool(torch.isfinite(f).all())
        seen = max(seen, float(f.abs().max()))
    print("walk with / without the DOF force tensor: max |d obs| %.3e, max |d reward| %.3e, max |tau| %.3e"
          % (dobs, drew, seen))
    assert seen > 0
    assert dobs <= 1e-5 and drew <= 1e-5, (dobs, drew)
