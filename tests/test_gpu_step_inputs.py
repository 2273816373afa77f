"""The humanoid step kernel's drive, limit and target inputs, which it loads
once per launch and holds in registers for every substep and for the
drive-clamp rerun (csrc/step_par.h, the three-round trees: 34 groups on 16
lanes).

Uniform properties cannot show a round of the lane reading another round's
registers, so every test here draws the properties per env and per DOF from a
fixed seed -- stiffness, damping, effort, armature, both joint limits and the
velocity limit, the DOFs of the third round (groups 32 and 33) included, with
one DOF per env pushed past a joint limit and a third of the DOFs faster than
their velocity limit -- on the thormang model set up as the walk task does
(tests/call_sequences.walk_sim), at 17 envs (a ragged second workgroup) and 32
(two full ones).

Parity is against the fp64 oracle stepped free-running from the same start:
the root and DOF state after every step under the walk parity bar, 1e-3 on
the observation (tests/gpu_harness.within) -- so each state quantity is
compared in the units the walk's observation carries it in (the cfg's
dofPositionScale 1, dofVelocityScale 0.05, linearVelocityScale 2,
angularVelocityScale 0.25; the root pose as it is).  Every start state and
every oracle trace is built once and shared."""
import functools

import numpy as np
import pytest
import torch

from tests import call_sequences as cs
from tests.oracle_lib import lib as oracle_lib, physics_step
from tests.test_gpu_dof_force import _h, _sp, pd_law
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.abi import (TG_PROP_ARMATURE, TG_PROP_DAMPING, TG_PROP_DRIVE_MODE, TG_PROP_EFFORT,
                                       TG_PROP_LOWER, TG_PROP_STIFFNESS, TG_PROP_UPPER, TG_PROP_VELOCITY)

pytestmark = pytest.mark.gpu

TOL = 1e-3   # the walk parity bar, on observation units
POS, VEL = 1, 2


@functools.lru_cache(None)
def _units():
    """(q, qd, root pose, root linear velocity, root angular velocity) -> observation units"""
    learn = _model()[2]["env"]["learn"]
    return (float(learn["dofPositionScale"]), float(learn["dofVelocityScale"]), 1.0,
            float(learn["linearVelocityScale"]), float(learn["angularVelocityScale"]))


def _obs_units(root, dof):
    """{quantity: the state in observation units (float64)}"""
    uq, uqd, up, ul, ua = _units()
    root, dof = root.astype(np.float64), dof.astype(np.float64)
    return {"q": uq * dof[:, 0], "qd": uqd * dof[:, 1], "pose": up * root[:, :7], "lin": ul * root[:, 7:10],
            "ang": ua * root[:, 10:13]}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


# ------------------------------------------------------------------ start states (CPU, cached, never modified)
@functools.lru_cache(None)
def _model():
    from thormang_isaacgym_amd.cfg import load_task_cfg
    from thormang_isaacgym_amd.sim import load_model
    m = load_model("thormang")
    return m, abi.ModelDesc(m), load_task_cfg("ThormangWalk", num_envs=1)


def _params(n, substeps):
    """The sim parameters as cs.walk_sim forms them."""
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_asset_options
    _, _, cfg = _model()
    sim_cfg = dict(cfg["sim"], substeps=substeps)
    return abi.sim_params_from_cfg(sim_cfg, walk_asset_options(cfg), n, float(cfg["env"].get("envSpacing", 1.0)),
                                   warn=False, default_contact_offset=0.016)


@functools.lru_cache(None)
def _start(n, substeps):
    """dict(sp, root [n,13], dof [n*D,2], props [P,n,D], pt, vt [n,D]): the
    walk's standing start with seeded joint offsets and velocities, and every
    drive, limit and target input distinct per (env, DOF).  Env e has DOF
    (D - 1 - e) mod D past a joint limit by 0.02 .. 0.05 rad (the upper one on
    even envs, the lower one on odd envs): envs 0 and 1 the last two DOFs, the
    third round's.  The DOFs with (e + d) mod 3 == 0 start at 1 .. 2 rad/s
    against a velocity limit of 0.3 .. 0.6 rad/s."""
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_dof_props
    m, _, cfg = _model()
    D = m.num_dof
    sp = _params(n, substeps)
    h = _h(sp)
    rs = np.random.default_rng(101)
    props, _, default = walk_dof_props(m, cfg, n)
    props = props.copy()
    root = np.zeros((n, 13), np.float32)
    root[:, 2] = float(cfg["env"].get("spawnHeight", 0.79))
    root[:, 6] = 1.0
    q = default[None, :] + rs.normal(0.0, 0.03, (n, D))
    qd = rs.uniform(-0.5, 0.5, (n, D))
    fast = (np.arange(n)[:, None] + np.arange(D)[None, :]) % 3 == 0
    qd = np.where(fast, rs.uniform(1.0, 2.0, (n, D)) * rs.choice([-1.0, 1.0], (n, D)), qd)
    props[TG_PROP_STIFFNESS] *= rs.uniform(0.5, 1.5, (n, D))
    props[TG_PROP_DAMPING] *= rs.uniform(0.5, 1.5, (n, D))
    props[TG_PROP_ARMATURE] = rs.uniform(0.005, 0.02, (n, D))
    props[TG_PROP_EFFORT] = rs.uniform(500.0, 1500.0, (n, D))
    props[TG_PROP_VELOCITY] = np.where(fast, rs.uniform(0.3, 0.6, (n, D)), rs.uniform(4.0, 9.0, (n, D)))
    qp = q + h * qd
    lo = np.minimum(props[TG_PROP_LOWER] - rs.uniform(0.0, 0.2, (n, D)), qp - 0.2)
    hi = np.maximum(props[TG_PROP_UPPER] + rs.uniform(0.0, 0.2, (n, D)), qp + 0.2)
    env = np.arange(n)
    past = (D - 1 - env) % D
    u = rs.uniform(0.02, 0.05, n)
    up = env % 2 == 0
    hi[env, past] = np.where(up, qp[env, past] - u, qp[env, past] + u + 1.0)
    lo[env, past] = np.where(up, qp[env, past] - u - 1.0, qp[env, past] + u)
    props[TG_PROP_LOWER], props[TG_PROP_UPPER] = lo, hi
    dof = np.stack([q, qd], axis=2).reshape(n * D, 2).astype(np.float32)
    pt = (default[None, :] + rs.uniform(-0.15, 0.15, (n, D))).astype(np.float32)
    vt = rs.uniform(-0.2, 0.2, (n, D)).astype(np.float32)
    st = dict(m=m, sp=sp, root=root, dof=dof, props=np.ascontiguousarray(props, np.float32), pt=pt, vt=vt)
    # the set-up is what the docstring says, on the float32 values the kernel reads
    qp32 = dof.reshape(n, D, 2)[..., 0].astype(np.float64) + h * dof.reshape(n, D, 2)[..., 1].astype(np.float64)
    out = np.maximum(st["props"][TG_PROP_LOWER] - qp32, qp32 - st["props"][TG_PROP_UPPER])
    assert (out[env, past] > 0.015).all() and ((out > 0).sum(axis=1) == 1).all()
    assert {D - 1, D - 2} <= set(past.tolist())
    for f in (TG_PROP_STIFFNESS, TG_PROP_DAMPING, TG_PROP_ARMATURE, TG_PROP_EFFORT, TG_PROP_LOWER, TG_PROP_UPPER,
              TG_PROP_VELOCITY):
        assert len(np.unique(st["props"][f])) > 0.9 * n * D, f
    assert (np.rint(st["props"][TG_PROP_DRIVE_MODE]) == POS).all()
    return st


def _with(st, **kw):
    return dict(st, **kw)


# ------------------------------------------------------------------ the two sides
def _oracle_trace(st, steps, precision="f64", sp=None):
    """[(root, dof)] after each of ``steps`` free-running control steps."""
    _, desc, _ = _model()
    root, dof = st["root"].copy(), st["dof"].copy()
    out = []
    for _ in range(steps):
        physics_step(desc, sp or st["sp"], root, dof, st["props"], st["pt"].copy(), st["vt"].copy(), threads=4,
                     L=oracle_lib(precision))
        out.append((root.copy(), dof.copy()))
    return out


def _load(sim, st):
    sim.root_state.copy_(torch.from_numpy(st["root"]))
    sim.dof_state.copy_(torch.from_numpy(st["dof"]))
    sim.dof_props.copy_(torch.from_numpy(st["props"]))
    sim.dof_vel_target.copy_(torch.from_numpy(st["vt"]))
    sim.set_dof_velocity_targets(sim.dof_vel_target)
    sim.set_dof_position_targets(torch.from_numpy(st["pt"]).to(cs.DEV))
    sim.env_dirty.fill_(1)
    sim.refresh()


def _gpu_trace(st, steps):
    n = st["root"].shape[0]
    sim = cs.walk_sim(n, substeps=int(st["sp"].substeps))
    assert not sim.jit
    _load(sim, st)
    out = []
    for _ in range(steps):
        sim.simulate()
        out.append((sim.root_state.cpu().numpy().copy(), sim.dof_state.cpu().numpy().copy()))
    sim.close()
    return out


def _compare(what, got, ref):
    """Per step and quantity the largest |GPU - fp64 oracle| in observation
    units, printed, then every one of them under TOL."""
    worst = {}
    for t, ((r1, d1), (r0, d0)) in enumerate(zip(got, ref)):
        assert np.isfinite(r1).all() and np.isfinite(d1).all() and np.isfinite(r0).all() and np.isfinite(d0).all()
        a1, a0 = _obs_units(r1, d1), _obs_units(r0, d0)
        e = {k: np.abs(a1[k] - a0[k]).max() for k in a1}
        print(what, "step %d:" % t, " ".join("%s %.3e" % kv for kv in e.items()))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
    assert len(got) == len(ref) and all(v < TOL for v in worst.values()), (what, worst)


# ------------------------------------------------------------------ 1. distinct properties
@functools.lru_cache(None)
def _plain_ref(n, substeps, steps):
    return _oracle_trace(_start(n, substeps), steps)


@pytest.mark.parametrize("n", [17, 32])
def test_distinct_inputs_per_env_and_dof_match_the_fp64_oracle(n):
    """2 substeps x 5 steps.  The inputs matter: with the velocity limits,
    the joint limits or the drive gains of each env's DOFs reversed in order
    the oracle's first step moves every env's DOF state by more than 4 TOL
    (twice what two sides that each meet the bar can differ by)."""
    _cuda()
    st = _start(n, 2)
    ref = _plain_ref(n, 2, 5)
    for fields in ((TG_PROP_VELOCITY,), (TG_PROP_LOWER, TG_PROP_UPPER), (TG_PROP_STIFFNESS, TG_PROP_DAMPING)):
        props = st["props"].copy()
        for f in fields:
            props[f] = props[f][:, ::-1]
        moved = _obs_units(*_oracle_trace(_with(st, props=props), 1)[0])
        base = _obs_units(*ref[0])
        eff = np.maximum(np.abs(moved["q"] - base["q"]), np.abs(moved["qd"] - base["qd"])).reshape(n, -1).max(axis=1)
        print("fields", fields, "reversed: per-env effect on the DOF state %.3e .. %.3e" % (eff.min(), eff.max()))
        assert eff.min() > 4 * TOL, (fields, float(eff.min()))
    _compare("distinct inputs, %d envs:" % n, _gpu_trace(st, 5), ref)


# ------------------------------------------------------------------ 2. clamp rerun
def _first_solve_ti(st, root, dof):
    """te - K qdd of a substep's first (all-implicit) solve from (root, dof)
    on the fp64 oracle: one substep with every effort 1e30, no velocity limit
    and the root lifted out of contact (the first solve comes before the
    contact solve and the velocity clip), ti by pd_law."""
    _, desc, _ = _model()
    props = st["props"].copy()
    props[TG_PROP_EFFORT] = 1e30
    props[TG_PROP_VELOCITY] = 0.0
    sp1 = _sp(st["sp"], substeps=1, dt=_h(st["sp"]))
    r, d = root.copy(), dof.copy()
    r[:, 2] += 10.0
    physics_step(desc, sp1, r, d, props, st["pt"].copy(), st["vt"].copy(), threads=4, L=oracle_lib("f64"))
    n = root.shape[0]
    return pd_law(_with(st, props=props), dof.reshape(n, -1, 2), d.reshape(n, -1, 2), _h(sp1))


@functools.lru_cache(None)
def _clamp_start(n):
    """_start with the targets of every third DOF 0.4 .. 0.7 rad further out
    and the efforts |ti| / 8 on those DOFs, 8 |ti| + 50 on the others, ti the
    first substep's first-solve torque.  Checked on the oracle, substep by
    substep (10 single-substep steps of h): in every substep every env has a
    drive at |ti| >= 2 effort, so the rerun runs in both substeps of every
    step."""
    st = _start(n, 2)
    m = st["m"]
    D = m.num_dof
    rs = np.random.default_rng(202)
    pick = np.arange(0, D, 3)
    pt = st["pt"].copy()
    pt[:, pick] += (rs.uniform(0.4, 0.7, (n, len(pick))) * rs.choice([-1.0, 1.0], (n, len(pick)))).astype(np.float32)
    st = _with(st, pt=pt)
    ti = np.abs(_first_solve_ti(st, st["root"], st["dof"]))
    sat = np.zeros((n, D), bool)
    sat[:, pick] = True
    props = st["props"].copy()
    props[TG_PROP_EFFORT] = np.where(sat, ti / 8, 8 * ti + 50).astype(np.float32)
    st = _with(st, props=props)
    eff = props[TG_PROP_EFFORT].astype(np.float64)
    assert (eff > 0).all()
    _, desc, _ = _model()
    sp1 = _sp(st["sp"], substeps=1, dt=_h(st["sp"]))
    root, dof = st["root"].copy(), st["dof"].copy()
    for k in range(10):
        r = np.abs(_first_solve_ti(st, root, dof)) / eff
        nsat = (r >= 2).sum(axis=1)
        print("clamp, %d envs, substep %d: saturated drives per env %d .. %d, entries with 0.5 < |ti| / effort < 2: %d"
              % (n, k, nsat.min(), nsat.max(), ((r > 0.5) & (r < 2)).sum()))
        assert nsat.min() >= 1, (k, int(nsat.min()))
        physics_step(desc, sp1, root, dof, st["props"], st["pt"].copy(), st["vt"].copy(), threads=4, L=oracle_lib("f64"))
    return st


@pytest.mark.parametrize("n", [17, 32])
def test_clamp_rerun_in_both_substeps_matches_the_fp64_oracle(n):
    """2 substeps x 5 steps with at least one saturated drive per env in
    every substep: pass 2a runs four times per launch on the held inputs."""
    _cuda()
    st = _clamp_start(n)
    _compare("clamp rerun, %d envs:" % n, _gpu_trace(st, 5), _oracle_trace(st, 5))


# ------------------------------------------------------------------ 3. substep count
@pytest.mark.parametrize("substeps", [1, 3])
def test_one_and_three_substeps_match_the_fp64_oracle(substeps):
    """32 envs, 3 steps."""
    _cuda()
    st = _start(32, substeps)
    _compare("%d substep(s):" % substeps, _gpu_trace(st, 3), _plain_ref(32, substeps, 3))


# ------------------------------------------------------------------ 4. writes between steps
W_ROW, W_VEL, W_LAST = 5, 9, 16   # envs written: a stiffness row, the velocity limits, a damping row (the ragged workgroup's env)


def _written_run(monkeypatch, write):
    """17 envs from _start: 2 simulates, then (``write``) a stiffness row, a
    damping row and the velocity limits of one env each through the zero-copy
    dof_props view, and new position targets; 2 more simulates.  With the
    writes, a fresh cache-free control sim gets everything the written sim
    holds at that point (cs.transplant: it has the new values from its first
    step) and runs the same two simulates.  Returns the traces of the last
    two simulates: the sim's, the control's (None without the writes)."""
    n = 17
    st = _start(n, 2)
    tg = cs.walk_targets(n, 4)
    sim = cs.walk_sim(n)
    _load(sim, st)
    for t in range(2):
        sim.set_dof_position_targets(tg[t])
        sim.simulate()
    ctl = None
    if write:
        sim.dof_props[TG_PROP_STIFFNESS, W_ROW] *= 0.5
        sim.dof_props[TG_PROP_DAMPING, W_LAST] *= 2.0
        sim.dof_props[TG_PROP_VELOCITY, W_VEL] = 0.05
        for e in (W_ROW, W_VEL, W_LAST):
            sim.env_dirty[e] = 1
        sim.refresh()
        ctl = cs.create_under(monkeypatch, cs.CONTROL, lambda: cs.walk_sim(n))
        cs.transplant(sim, ctl)
    traces = []
    for s in (sim, ctl):
        if s is None:
            traces.append(None)
            continue
        tr = []
        for t in (2, 3):
            s.set_dof_position_targets(tg[t])
            s.simulate()
            tr.append(cs.snap_sim(s))
        s.sync()
        s.close()
        traces.append(tr)
    return traces


def test_writes_between_steps_take_effect_at_the_next_step(monkeypatch):
    """Bit for bit the control's states; and against the same run without
    the writes exactly the written envs differ after the next step."""
    _cuda()
    a, ctl = _written_run(monkeypatch, True)
    b, _ = _written_run(monkeypatch, False)
    cs.assert_same(a, ctl, "written sim vs the control that had the values from its first step")
    moved = cs.changed_envs(a[0], b[0], 17)
    assert moved == {W_ROW, W_VEL, W_LAST}, sorted(moved)
