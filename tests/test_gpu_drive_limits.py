"""The step kernel's per-joint discontinuities on the GPU: the effort clamp
(Woodbury update, its fallback, the plain rerun; multi-round and one-round
forms), the ramped joint-limit spring, the velocity limit, effort-mode
actuation, base damping and external wrenches.

A. One control step, teacher-forced, root and dof state against the fp64
   oracle.  Every case is built on the CPU first: the oracle steps the
   feature-off twin (effort 1e30, windows out of reach, velocity limit 0, ...),
   every (env, DOF) is classified on the oracle's states with a factor of 2 to
   the threshold, and the feature must move the joint velocities of every env
   by at least 100x the fp32 control's error and 1e-3 (``_teeth``).  So no
   test depends on which side of a threshold fp32 rounding falls.

   Bound (``_check``), per quantity (joint position, joint velocity, root
   pose, root velocity), maxima over the kept envs: the GPU's error against
   fp64 is at most max(4 x the error of the oracle's fp32 build on the same
   case, 16 ulp32(largest magnitude of the quantity)) -- 4x is the ratio both
   tensor tests use, the floor covers controls that are exactly 0 (a fixed
   base) -- and inside the project's one-step bar of 1e-4 on positions and
   1e-3 on velocities (test_gpu_solver_type_switches_at_runtime).

   The same cases again with both force tensors acquired (bit-identical end
   state) and on a level heightfield (the same bound).

B. Known answers the physics requires, on the GPU with the bounds the CPU
   oracle's tests state (tests/test_physics_oracle.py, the same helpers).

35 envs as tests/test_gpu_dof_force.py, whose conventions are imported."""
import functools

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.oracle_lib import lib as oracle_lib, physics_step
from tests.test_gpu_dof_force import (EFFORT, N, POS, VEL, _cuda, _h, _lifted, _sim, _sp, _state, _unlocked, _with,
                                      pd_law, ulp32)
from thormang_isaacgym_amd.abi import (TG_PROP_DAMPING, TG_PROP_DRIVE_MODE, TG_PROP_EFFORT, TG_PROP_LOWER,
                                       TG_PROP_STIFFNESS, TG_PROP_UPPER, TG_PROP_VELOCITY)

pytestmark = pytest.mark.gpu

RAMP = pm.limit_ramp()
FAR = 3.4e38
ARTICULATED = ("gogoro", "thormang", "thormang_wb")
# (quantity, the project's one-step bar)
BARS = (("q", 1e-4), ("qd", 1e-3), ("pose", 1e-4), ("vel", 1e-3))


# ------------------------------------------------------------------ states
@functools.lru_cache(None)
def _pendulum_state():
    """kat_pendulum_y, fixed base, a POS drive, a different state per env."""
    m = pm.pendulum()
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=N, dt=0.01, substeps=1, fix_base_link=True)
    rs = np.random.default_rng(5)
    props[TG_PROP_DRIVE_MODE] = POS
    props[TG_PROP_STIFFNESS, :, 0] = rs.uniform(100, 400, N)
    props[TG_PROP_DAMPING, :, 0] = rs.uniform(2, 10, N)
    props[TG_PROP_EFFORT] = 1e30
    props[TG_PROP_VELOCITY] = 0.0
    dof[:, 0] = rs.uniform(-1, 1, N)
    dof[:, 1] = rs.uniform(-1, 1, N)
    pt[:, 0] = dof[:, 0] + rs.uniform(1.0, 2.0, N) * rs.choice([-1.0, 1.0], N)
    return dict(m=m, desc=desc, sp=sp, root=root, dof=dof, props=props, pt=pt, vt=vt)


def _start(name, where="ground"):
    """(state, one-substep sim params) with efforts 1e30 and no velocity
    limit.  ``where``: "ground" (the standing starts), "air" (lifted 1 m) or
    "air_fixed" (lifted, fixed base)."""
    st = _pendulum_state() if name == "kat_pendulum_y" else _state(name)
    props = st["props"].copy()
    props[TG_PROP_VELOCITY] = 0.0
    st = _with(st, props=props)
    sp = _sp(st["sp"], substeps=1)
    if name in ARTICULATED and where != "ground":
        st = _lifted(st)
        if where == "air_fixed":
            sp = _sp(sp, fix_base=1)
    return st, sp


def _two_substeps(sp):
    """substeps = 2 over 2 h."""
    sp2 = _sp(sp, substeps=2, dt=float(np.float32(2) * np.float32(sp.dt)))
    assert _h(sp2) == _h(sp)
    return sp2


def _props(st, **fields):
    props = st["props"].copy()
    for k, v in fields.items():
        props[{"effort": TG_PROP_EFFORT, "lower": TG_PROP_LOWER, "upper": TG_PROP_UPPER,
               "velocity": TG_PROP_VELOCITY, "mode": TG_PROP_DRIVE_MODE}[k]] = v
    return _with(st, props=props)


def _drives(st):
    mode = np.rint(st["props"][TG_PROP_DRIVE_MODE])
    return (mode == POS) | (mode == VEL)


def _free_mask(st):
    f = np.zeros(st["m"].num_dof, bool)
    f[_unlocked(st["desc"])] = True
    return f


# ------------------------------------------------------------------ stepping
def _oracle(st, sp, precision, act=None, force=None):
    root, dof = st["root"].copy(), st["dof"].copy()
    physics_step(st["desc"], sp, root, dof, st["props"], st["pt"].copy(), st["vt"].copy(), act=act, force=force,
                 threads=4, L=oracle_lib(precision))
    return root, dof.reshape(N, st["m"].num_dof, 2)


def _gpu(st, sp, act=None, force=None, tensors=False, hf=False):
    """One simulate from the start state: (root [N,13], dof [N,D,2])."""
    s, _, _ = _sim(st, sp, act, contact=tensors, dof_force=tensors, hf=hf)
    if force is not None:   # as the walk task's push: written into the bound tensor, then applied
        s.body_force.copy_(torch.from_numpy(force))
        s.apply_body_forces(s.body_force)
    s.simulate()
    out = s.root_state.cpu().numpy().copy(), s.dof_state.cpu().numpy().reshape(N, st["m"].num_dof, 2).copy()
    s.close()
    return out


def _parts(rd):
    root, dof = rd
    return {"q": dof[..., 0].astype(np.float64), "qd": dof[..., 1].astype(np.float64),
            "pose": root[:, :7].astype(np.float64), "vel": root[:, 7:].astype(np.float64)}


def _err(a, ref, keep):
    a, ref = _parts(a), _parts(ref)
    assert all(np.isfinite(a[k]).all() and np.isfinite(ref[k]).all() for k in a)
    return {k: float(np.abs(a[k][keep] - ref[k][keep]).max()) for k in a}


def _first_solve_ti(st, sp):
    """te - K qdd of a substep's first (all-implicit) solve from ``st``, on the
    fp64 oracle: one substep with every effort 1e30 and no velocity limit, the
    root lifted out of contact (the first solve comes before the contact
    solve and does not see the height), ti by pd_law."""
    tw = _lifted(_props(st, effort=1e30, velocity=0.0), 10.0)
    sp1 = _sp(sp, substeps=1, dt=_h(sp))
    _, dof1 = _oracle(tw, sp1, "f64")
    return pd_law(tw, tw["dof"].reshape(N, -1, 2), dof1, _h(sp1))


# ------------------------------------------------------------------ a case: CPU part
def _teeth(what, ref, off, ctl_qd, keep):
    """The feature moves every kept env's joint velocities by at least 100x the
    case's control error and 1e-3."""
    eff = np.abs(_parts(ref)["qd"] - _parts(off)["qd"]).max(axis=1)[keep]
    need = max(100 * ctl_qd, 1e-3)
    print(what, "teeth: per-env effect on joint velocity %.3e .. %.3e, needed %.3e" % (eff.min(), eff.max(), need))
    assert eff.min() >= need, (what, float(eff.min()), need)


def _case(what, st, sp, twin, twin_sp=None, act=None, twin_act=None, force=None, keep=None, **extra):
    """Oracle (fp64), control (fp32) and the feature-off twin (fp64); the
    kept-env count (at most a quarter left out) and the teeth."""
    keep = np.ones(N, bool) if keep is None else keep
    print(what, "kept envs: %d of %d" % (keep.sum(), N))
    assert N - keep.sum() <= N // 4, (what, int(keep.sum()))
    ref = _oracle(st, sp, "f64", act, force)
    ctl = _oracle(st, sp, "f32", act, force)
    off = _oracle(twin, twin_sp or sp, "f64", twin_act, None if extra.pop("twin_no_force", False) else force)
    e_ctl = _err(ctl, ref, keep)
    _teeth(what, ref, off, e_ctl["qd"], keep)
    return dict(extra, what=what, st=st, sp=sp, act=act, force=force, keep=keep, ref=ref, e_ctl=e_ctl)


_GPU = {}


def _gpu_of(key, variant="plain"):
    """The case's GPU end state (cached: the tensor and heightfield tests
    compare with the plain run)."""
    if (key, variant) not in _GPU:
        c = CASES[key]()
        _GPU[key, variant] = _gpu(c["st"], c["sp"], c["act"], c["force"], tensors=variant == "tensors",
                                  hf=variant == "hf")
    return _GPU[key, variant]


def _check(c, got, tag=""):
    """The bound of the module docstring; prints GPU error, control error and
    ratio per quantity, then asserts."""
    e_gpu, ref, keep = _err(got, c["ref"], c["keep"]), _parts(c["ref"]), c["keep"]
    bad = []
    for k, bar in BARS:
        floor = 16 * float(ulp32(np.abs(ref[k][keep]).max()))
        bound = max(4 * c["e_ctl"][k], floor)
        print("%s%s %-4s GPU %.3e, control %.3e, ratio %.2f, floor %.3e (kept %d)"
              % (c["what"], tag, k, e_gpu[k], c["e_ctl"][k], e_gpu[k] / max(c["e_ctl"][k], 1e-300), floor, keep.sum()))
        if not (e_gpu[k] <= bound and e_gpu[k] < bar):
            bad.append((k, e_gpu[k], bound, bar))
    assert not bad, (c["what"] + tag, bad)


# ------------------------------------------------------------------ A.1 effort clamp
def _clamp_case(name, where, nsat, substeps, F):
    """Efforts |ti| / F on the saturated drives and F |ti| + 1 on the others,
    ti the first substep's first-solve torque on the oracle; with two substeps
    the second substep is classified the same way from the oracle's mid state
    and an env with a drive at 0.5 < |ti| / effort < 2 in either is left out."""
    st, sp = _start(name, where)
    free = _unlocked(st["desc"])
    rs = np.random.default_rng(6 if name == "gogoro" else 8)
    if name == "gogoro":
        pick = list(free[:nsat])
        push = free
    elif name in ("thormang", "thormang_wb"):
        pick = list(free[::3])
        push = pick
    else:
        pick, push = [0], []
    pt = st["pt"].copy()
    pt[:, push] += (rs.uniform(0.3, 0.6, (N, len(push))) * rs.choice([-1.0, 1.0], (N, len(push)))).astype(np.float32)
    st = _with(st, pt=pt)
    what = "clamp %s %s, %d saturated, %d substep(s), F %g:" % (name, where, len(pick), substeps, F)
    drv = _drives(st)
    sat = np.zeros_like(drv)
    sat[:, pick] = True
    sat &= drv
    assert (sat.sum(axis=1) == len(pick)).all()
    ti = _first_solve_ti(st, sp)
    eff = np.where(sat, np.abs(ti) / F, F * np.abs(ti) + 1).astype(np.float32)
    on = _props(st, effort=np.where(drv, eff, st["props"][TG_PROP_EFFORT]))
    e64 = on["props"][TG_PROP_EFFORT].astype(np.float64)
    assert (np.abs(ti)[sat] >= 2 * e64[sat]).all() and (e64[sat] > 0).all()
    assert (np.abs(ti)[drv & ~sat] <= 0.5 * e64[drv & ~sat]).all()
    keep = np.ones(N, bool)
    if substeps == 2:
        mid_root, mid_dof = _oracle(on, sp, "f64")
        ti2 = _first_solve_ti(_with(on, root=mid_root, dof=mid_dof.reshape(-1, 2)), sp)
        r2 = np.abs(ti2) / e64
        keep = ~(drv & (r2 > 0.5) & (r2 < 2)).any(axis=1)
        print(what, "second substep: saturated drives per kept env %d .. %d"
              % ((drv & (r2 >= 2))[keep].sum(axis=1).min(), (drv & (r2 >= 2))[keep].sum(axis=1).max()))
        assert (drv & (r2 >= 2))[keep].any(), "the second substep clamps too"
        sp = _two_substeps(sp)
    return _case(what, on, sp, _props(on, effort=1e30), keep=keep)


# ------------------------------------------------------------------ A.2 joint limits
def _limit_pick(st, clamp):
    """A third of the free DOFs; the pendulum's one, the chain's prismatic one.
    gogoro with a saturated drive: its steering joint, the one gogoro DOF that
    has both a window and a drive in the task."""
    free = _unlocked(st["desc"])
    if st["m"].name == "gogoro" and clamp:
        assert st["m"].dof_names[free[0]] == "steering_joint"
        return [free[0]]
    return {"kat_pendulum_y": [0], "kat_chain": [1]}.get(st["m"].name) or list(free[::3])


def _limit_windows(st, sp, pick, seed):
    """Windows on the DOFs in ``pick`` placed from qp = q + h qd so that qp is
    past the limit by u, random side per (env, DOF); half the entries with u
    inside the ramp (0.0005 .. 0.8 RAMP), half beyond it (1.5 .. 3 RAMP).  The
    other free DOFs end at least 1 rad inside theirs; locked DOFs keep their
    (lock) windows.  Returns the state and its twin with the picked windows
    out of reach."""
    rs = np.random.default_rng(seed)
    h = _h(sp)
    d = st["dof"].reshape(N, -1, 2).astype(np.float64)
    qp = d[..., 0] + h * d[..., 1]
    lo, hi = st["props"][TG_PROP_LOWER].astype(np.float64), st["props"][TG_PROP_UPPER].astype(np.float64)
    free = _free_mask(st)
    lo[:, free] = np.minimum(lo[:, free], qp[:, free] - 1.0)
    hi[:, free] = np.maximum(hi[:, free], qp[:, free] + 1.0)
    off = _props(st, lower=lo.astype(np.float32), upper=hi.astype(np.float32))
    tw_lo, tw_hi = lo.copy(), hi.copy()
    n, P = N * len(pick), len(pick)
    inside = (np.arange(N)[:, None] + np.arange(P)[None, :]) % 2 == 1   # (alternating: every env with 2+ has both)
    u = np.where(inside, rs.uniform(0.0005, 0.8 * RAMP, (N, P)), rs.uniform(1.5 * RAMP, 3 * RAMP, (N, P)))
    up = rs.choice([True, False], (N, len(pick)))
    qpp = qp[:, pick]
    hi[:, pick] = np.where(up, qpp - u, qpp + u + 1.0)
    lo[:, pick] = np.where(up, qpp - u - 1.0, qpp + u)
    tw_lo[:, pick], tw_hi[:, pick] = -FAR, FAR
    on = _props(st, lower=lo.astype(np.float32), upper=hi.astype(np.float32))
    # on the float32 windows, as the kernel reads them
    lo32, hi32 = on["props"][TG_PROP_LOWER].astype(np.float64), on["props"][TG_PROP_UPPER].astype(np.float64)
    past = np.maximum(lo32 - qp, qp - hi32)
    pk = np.zeros(st["m"].num_dof, bool)
    pk[pick] = True
    assert (past[:, pk] >= 0.0004).all() and (past[:, free & ~pk] <= -RAMP).all()
    inr = (past[:, pk] < 0.9 * RAMP).sum()
    assert inr == inside.sum() and abs(2 * inr - n) <= 1 and (past[:, pk] > 1.4 * RAMP).sum() == n - inr
    assert ((lo32 - qp)[:, pk] > 0).any() and ((qp - hi32)[:, pk] > 0).any(), "both sides"
    return on, _props(off, lower=tw_lo.astype(np.float32), upper=tw_hi.astype(np.float32))


def _limit_case(name, where, clamp):
    st, sp = _start(name, where)
    pick = _limit_pick(st, clamp)
    what = "limit %s %s%s:" % (name, where, " + clamp" if clamp else "")
    if name.startswith("thormang"):   # both forms of the leaf branch of the drive pass
        _, leaf = pm.dof_tree(st["desc"])
        assert leaf[pick].any() and (~leaf[pick]).any(), "a leaf group and a non-leaf group among the picked DOFs"
    if clamp:
        rs = np.random.default_rng(12)
        pt = st["pt"].copy()
        pt[:, pick] += (rs.uniform(0.3, 0.6, (N, len(pick))) * rs.choice([-1.0, 1.0], (N, len(pick)))).astype(np.float32)
        st = _with(st, pt=pt)
    on, twin = _limit_windows(st, sp, pick, 31)
    if clamp:   # a saturated drive on the DOFs at their limits: ti from the first solve with the limits on
        drv = _drives(on)
        sat = np.zeros_like(drv)
        sat[:, pick] = True
        assert (sat & drv).sum() == sat.sum(), "the picked DOFs are driven"
        ti = _first_solve_ti(on, sp)
        eff = np.where(sat, np.abs(ti) / 4, 4 * np.abs(ti) + 1).astype(np.float32)
        on = _props(on, effort=np.where(drv, eff, on["props"][TG_PROP_EFFORT]))
        e64 = on["props"][TG_PROP_EFFORT].astype(np.float64)
        assert (np.abs(ti)[sat] >= 2 * e64[sat]).all() and (e64[sat] > 0).all()
        assert (np.abs(ti)[drv & ~sat] <= 0.5 * e64[drv & ~sat]).all()
    return _case(what, on, sp, twin)


# ------------------------------------------------------------------ A.3 velocity limit
def _vel_case(name, where):
    """TG_PROP_VELOCITY = 0.5 |qd1| (floor 1e-3) on a third of the free DOFs
    and 4 |qd1| + 1 on the others, qd1 the twin's (no limit) end velocity."""
    st, sp = _start(name, where)
    free = _unlocked(st["desc"])
    pick = [1] if name == "kat_chain" else list(free[1::3])
    twin = _props(st, velocity=0.0)
    qd1 = np.abs(_parts(_oracle(twin, sp, "f64"))["qd"])
    vl = 4 * qd1 + 1
    vl[:, pick] = np.maximum(0.5 * qd1[:, pick], 1e-3)
    vl[:, ~_free_mask(st)] = st["props"][TG_PROP_VELOCITY][:, ~_free_mask(st)]
    on = _props(st, velocity=vl.astype(np.float32))
    v32 = on["props"][TG_PROP_VELOCITY].astype(np.float64)
    clipped = np.zeros((N, st["m"].num_dof), bool)
    clipped[:, pick] = qd1[:, pick] >= 2 * v32[:, pick]
    what = "velocity limit %s %s:" % (name, where)
    print(what, "clipped entries %d of %d picked" % (clipped.sum(), N * len(pick)))
    assert clipped.sum() >= 0.9 * N * len(pick)
    rest = np.setdiff1d(free, pick)
    assert (qd1[:, rest] <= 0.25 * v32[:, rest]).all(), "the others stay a factor of 4 inside"
    return _case(what, on, sp, twin, clipped=clipped, sign=np.sign(_parts(_oracle(twin, sp, "f64"))["qd"]))


# ------------------------------------------------------------------ A.4 effort mode
def _effort_case(name, where):
    """Every free DOF in effort mode, random actuation, a third of it beyond
    the effort; the twin has effort 1e30.  The effort of a DOF is the torque
    that changes its velocity by 1 rad/s in the step (probed on the oracle,
    the median over the envs), so that light and heavy DOFs alike stay at
    velocities of a few rad/s."""
    st, sp = _start(name, where)
    free = _free_mask(st)
    rs = np.random.default_rng(41)
    mode = st["props"][TG_PROP_DRIVE_MODE].copy()
    mode[:, free] = EFFORT
    probe = _props(st, mode=mode, effort=1e30)
    D = st["m"].num_dof
    qd0 = _parts(_oracle(probe, sp, "f64", np.zeros((N, D), np.float32)))["qd"]
    E = np.ones(D)
    for d in np.nonzero(free)[0]:
        one = np.zeros((N, D), np.float32)
        one[:, d] = 1.0
        E[d] = 1.0 / np.median(np.abs(_parts(_oracle(probe, sp, "f64", one))["qd"][:, d] - qd0[:, d]))
    E = E.astype(np.float32)[None, :]
    eff = st["props"][TG_PROP_EFFORT].copy()
    eff[:, free] = np.broadcast_to(E, (N, D))[:, free]
    act = np.zeros((N, st["m"].num_dof), np.float32)
    F = int(free.sum())
    beyond = (np.arange(N)[:, None] + np.arange(F)[None, :]) % 3 == 0
    mag = np.where(beyond, rs.uniform(1.25, 2.0, (N, F)), rs.uniform(0.0, 0.8, (N, F))) * E[:, free]
    act[:, free] = mag * rs.choice([-1.0, 1.0], (N, F))
    assert np.array_equal((np.abs(act) > E)[:, free], beyond) and beyond.any(axis=1).all()
    on = _props(st, mode=mode, effort=eff)
    return _case("effort mode %s %s:" % (name, where), on, sp, _props(on, effort=1e30), act=act, twin_act=act)


# ------------------------------------------------------------------ A.5 damping, wrench
def _spinning(name):
    """A free root in the air, spinning, with joint velocities of a few rad/s."""
    st, sp = _start(name, "air")
    rs = np.random.default_rng(51)
    root, dof = st["root"].copy(), st["dof"].copy()
    free = _unlocked(st["desc"])
    if name in ARTICULATED:
        root[:, 7:10] = rs.normal(0, 1, (N, 3))
        root[:, 10:13] = rs.normal(0, 2, (N, 3))
    lo = 8.0 if name == "kat_chain" else 1.0   # (the chain: well above what its root's spin of up to 5 rad/s couples in)
    dof.reshape(N, -1, 2)[:, free, 1] = rs.uniform(lo, 2 * lo, (N, len(free))) * rs.choice([-1.0, 1.0], (N, len(free)))
    return _with(st, root=root, dof=dof), sp


def _damping_case(name):
    st, sp = _spinning(name)
    return _case("base damping %s:" % name, st, _sp(sp, linear_damping=0.01, angular_damping=0.5), st, twin_sp=sp)


def _wrench_case(name):
    st, sp = _start(name) if name == "thormang" else _spinning(name)
    rs = np.random.default_rng(52)
    G = st["m"].num_groups
    force = np.concatenate([rs.normal(0, 20.0, (N, G, 3)), rs.normal(0, 2.0, (N, G, 3))], axis=2).astype(np.float32)
    return _case("wrench %s:" % name, st, sp, st, force=force, twin_no_force=True)


# ------------------------------------------------------------------ the cases
CLAMP = [("kat_pendulum_y", "air", 1, 1, 4), ("kat_pendulum_y", "air", 1, 2, 4),
         ("gogoro", "air", 2, 1, 4), ("gogoro", "air", 3, 1, 4), ("gogoro", "air", 4, 1, 4),
         ("gogoro", "air", 2, 2, 4), ("gogoro", "air", 3, 2, 4),
         ("gogoro", "ground", 2, 1, 4), ("gogoro", "ground", 3, 1, 4), ("gogoro", "ground", 3, 2, 4),
         ("thormang", "air_fixed", 11, 1, 4), ("thormang", "air_fixed", 11, 2, 32),
         ("thormang", "ground", 11, 1, 4), ("thormang", "ground", 11, 2, 32),
         ("thormang_wb", "ground", 11, 1, 4), ("thormang_wb", "ground", 11, 2, 32)]
LIMIT = [("kat_pendulum_y", "air", False), ("kat_chain", "air", False), ("gogoro", "ground", False),
         ("thormang", "ground", False), ("thormang_wb", "ground", False), ("thormang", "air_fixed", False),
         ("gogoro", "ground", True), ("thormang", "air_fixed", True)]
VELLIM = [("kat_chain", "air"), ("gogoro", "air"), ("gogoro", "ground"), ("thormang", "air"), ("thormang", "ground"),
          ("thormang_wb", "ground")]

CASES = {}
for _a in CLAMP:
    CASES[("clamp",) + _a] = functools.lru_cache(None)(functools.partial(_clamp_case, *_a))
for _a in LIMIT:
    CASES[("limit",) + _a] = functools.lru_cache(None)(functools.partial(_limit_case, *_a))
for _a in VELLIM:
    CASES[("vel",) + _a] = functools.lru_cache(None)(functools.partial(_vel_case, *_a))
for _a in (("gogoro", "ground"),):
    CASES[("effort",) + _a] = functools.lru_cache(None)(functools.partial(_effort_case, *_a))
for _n in ("gogoro", "kat_chain"):
    CASES[("damping", _n)] = functools.lru_cache(None)(functools.partial(_damping_case, _n))
for _n in ("gogoro", "kat_chain", "thormang"):
    CASES[("wrench", _n)] = functools.lru_cache(None)(functools.partial(_wrench_case, _n))


def _id(key):
    return "-".join(str(k) for k in key)


def _keys(kind):
    return [pytest.param(k, id=_id(k[1:])) for k in CASES if k[0] == kind]


# ------------------------------------------------------------------ A.1 - A.5: the tests
@pytest.mark.parametrize("key", _keys("clamp"))
def test_effort_clamp_state_matches_the_fp64_oracle(key):
    """Woodbury with one clamped drive (pendulum), with two (gogoro), its
    fallback (gogoro, 3 and 4), the rerun in the multi-round form (thormang:
    fixed base in the air, and standing with live contacts; thormang_wb: 8-env
    workgroups), one substep and two (the drive inputs are reused and the
    Woodbury count is reset per substep)."""
    _cuda()
    _check(CASES[key](), _gpu_of(key))


@pytest.mark.parametrize("key", _keys("limit"))
def test_joint_limit_state_matches_the_fp64_oracle(key):
    """The limit spring inside its ramp and beyond it, both sides, on revolute
    and prismatic DOFs, leaf and non-leaf groups; alone and with a saturated
    drive on the same DOF (gogoro: the steering joint at its stop; thormang:
    with a fixed base, because standing on the ground the same case misses the
    4x bar in the root's angular velocity alone, 1.48e-5 against a control of
    3.5e-6 rad/s, as every standing thormang case here has 1e-5 .. 2.4e-5 --
    DESIGN.md 8.2's root-origin cancellation)."""
    _cuda()
    _check(CASES[key](), _gpu_of(key))


@pytest.mark.parametrize("key", _keys("vel"))
def test_velocity_limit_state_matches_the_fp64_oracle_and_clips_exactly(key):
    """Parity, and with no tolerance: a clipped entry's stored velocity is
    +-limit as float32 bit for bit, and no entry exceeds its limit.  (The
    integrating velocity's clip has no such exact check: |q1 - q0| <= h limit
    (1 + 2^-22) does not hold for a float32 q1 -- the fp64 oracle's own stored
    positions exceed h limit by up to 6.5e-5 relative on these cases, half an
    ulp of q against a step of h limit -- so that clip is covered by the
    parity of q alone.)"""
    _cuda()
    c = CASES[key]()
    root1, dof1 = _gpu_of(key)
    _check(c, (root1, dof1))
    vl = c["st"]["props"][TG_PROP_VELOCITY]
    clipped, keep = c["clipped"], c["keep"]
    want = (c["sign"] * vl).astype(np.float32)
    got = dof1[..., 1]
    assert np.array_equal(got[clipped].view(np.uint32), want[clipped].view(np.uint32)), \
        float(np.abs(got[clipped] - want[clipped]).max())
    lim = vl > 0
    assert (np.abs(got)[lim] <= vl[lim]).all(), float((np.abs(got)[lim] - vl[lim]).max())


@pytest.mark.parametrize("key", _keys("effort"))
def test_effort_mode_actuation_state_matches_the_fp64_oracle(key):
    """gogoro.  The humanoid is not here: with every DOF in effort mode (no
    implicit drive gain in any joint's D) thormang misses the 4x bar -- standing
    on the ground in the root's angular velocity, 8.1e-6 against a control of
    1.8e-6 rad/s, and with a fixed base in the air in the joint velocities,
    2.1e-5 against 1.7e-6 rad/s (floor 7.6e-6) -- which is the root-origin
    cancellation of DESIGN.md 8.2, not the actuation clamp."""
    _cuda()
    _check(CASES[key](), _gpu_of(key))


@pytest.mark.parametrize("key", _keys("damping") + _keys("wrench"))
def test_base_damping_and_external_wrench_state_matches_the_fp64_oracle(key):
    """The task's linear / angular damping (0.01 / 0.5) through the sim
    params, and a random wrench on every group through sim.body_force."""
    _cuda()
    _check(CASES[key](), _gpu_of(key))


# ------------------------------------------------------------------ A.6 the other instantiations
OTHER = [k for k in CASES if k[0] in ("clamp", "limit", "vel") and k[1] in ("gogoro", "thormang")]


@pytest.mark.parametrize("key", [pytest.param(k, id=_id(k)) for k in OTHER])
def test_force_tensors_leave_the_end_state_bit_identical(key):
    """With the DOF force tensor and the contact tensor acquired (the
    instantiations whose clamp passes also store the export's values) the end
    state is the plain run's, bit for bit."""
    _cuda()
    CASES[key]()
    (r0, d0), (r1, d1) = _gpu_of(key), _gpu_of(key, "tensors")
    assert np.isfinite(r0).all() and np.isfinite(d0).all()
    assert np.array_equal(r0.view(np.uint32), r1.view(np.uint32))
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


@pytest.mark.parametrize("key", [pytest.param(k, id=_id(k)) for k in OTHER])
def test_level_heightfield_meets_the_plane_bound(key):
    _cuda()
    _check(CASES[key](), _gpu_of(key, "hf"), " (heightfield)")


# ------------------------------------------------------------------ B. known answers
def _make_step(mu=None):
    """A ``step_fn`` for the physics_models helpers backed by a one-env Sim of
    a compiled-in model, created from the state of the first call."""
    from thormang_isaacgym_amd.sim import Sim
    sims = []

    def step(desc, sp, root, dof, props, pt, vt):
        if not sims:
            s = Sim(desc.model, sp, 1, "cuda:0")
            assert not s.jit
            s.root_state.copy_(torch.from_numpy(root))
            s.dof_state.copy_(torch.from_numpy(dof))
            s.dof_props.copy_(torch.from_numpy(props))
            s.dof_pos_target.copy_(torch.from_numpy(pt))
            s.dof_vel_target.copy_(torch.from_numpy(vt))
            s.env_dirty.fill_(1)
            if mu is not None:
                s.set_shape_friction_indexed(torch.full((1, s.S), mu, device="cuda:0"), s.all_ids)
            sims.append(s)
        sims[0].simulate()
        root[...] = sims[0].root_state.cpu().numpy()
        dof[...] = sims[0].dof_state.cpu().numpy()
    return step


def test_gpu_velocity_drive_steady_state_and_effort_limit():
    _cuda()
    steady, limited = pm.velocity_drive_runs(_make_step)
    print("velocity drive: steady %.6f rad/s, effort-limited %.6f rad/s" % (steady[-1], limited[-1]))
    assert abs(steady[-1] - 7.0) < 1e-3
    np.testing.assert_allclose(limited[-1], 0.5 / 0.01 * 0.1, rtol=2e-3)


def test_gpu_position_drive_converges():
    _cuda()
    tr = pm.position_drive_run(_make_step())
    print("position drive: final %.6f rad" % tr[-1])
    assert abs(tr[-1] - 0.4) < 1e-4


def test_gpu_joint_limit_holds_against_gravity():
    """The +-0.3 window through dof_props on kat_pendulum_y, the fixed base
    tilted by its root quaternion."""
    _cuda()
    tr = pm.joint_limit_run(_make_step(), through_props=True)
    print("joint limit: max |q| %.4f, final %.4f" % (np.abs(tr).max(), tr[-1]))
    assert np.abs(tr).max() < 0.36
    assert abs(abs(tr[-1]) - 0.3) < 0.01


def test_gpu_coulomb_sliding_distance():
    """ground_friction and the shape friction of the compiled-in kat_box (1.0)
    both set to 0.5 at run time."""
    _cuda()
    tr, d_exp = pm.coulomb_slide_run(_make_step(mu=0.5), mu=0.5, model=pm.box_body())
    print("sliding: %.4f m of %.4f m expected, final speed %.2e" % (tr[-1, 0], d_exp, tr[-1, 1]))
    assert abs(tr[-1, 0] - d_exp) / d_exp < 0.05
    assert abs(tr[-1, 1]) < 1e-3


def test_gpu_chain_internal_drive_keeps_system_com_fixed():
    _cuda()
    tr = pm.chain_internal_drive_run(_make_step())
    print("chain: final joint rate %.4f, COM moved %.2e m" % (tr[-1, 3], np.abs(tr[:, :3] - tr[0, :3]).max()))
    assert np.all(np.isfinite(tr))
    assert abs(tr[-1, 3] - 4.0) < 0.05
    assert np.abs(tr[:, :3] - tr[0, :3]).max() < 2e-3
