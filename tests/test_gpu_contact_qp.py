"""Contact forces inside friction cones on the GPU (tg_contact_qp, Sim.contact_qp)
against the float64 reference of tests/contact_qp_ref.py (pinned by
tests/test_contact_qp_reference.py), run for the same number of iterations.

Eight envs, env 1 far out on the grid at (300, -200, 1).  thormang: the
ThormangWalk default stance with joint angles off by U(-0.1, 0.1) rad, a root
tilt of a few degrees, random root and joint velocities, on both soles
(walk_sole_patch); gogoro: upright with random joint states on two point
contacts.  Every sim with a body mass scale U(0.8, 1.2) per link and an armature
U(0.005, 0.02) per DOF, the outputs filled with NaN before each call.

Tolerance.  Per model, max |x - x_ref| over the largest force of the case (max
|b[:, 0:3]|: forces, wrench forces, tau[:, 0:3], info[:, 0]) and over its largest
torque (max |b[:, 3:]|: wrench moments, tau[:, 3:], info[:, 1]), <= 4 x the worst
value measured on the MI355X over every comparison of this file (QP_MEASURED
below; profiles/r13/contact_qp_parity.txt has the per-case figures), under 5e-3,
above which a difference is a bug and not rounding.  info[:, 3] (the loaded
vertices) may differ where a reference normal force is within the tolerance of
0, on at most 2 % of the vertices of a call; the float32 run of the reference is
held to the same.

Always feasible.  Every call of this file checks the device's own forces: f.n >=
0 and |f_t| <= mu f.n (1 + 1e-5) + 1e-5 with the float64 unit normals.  One
sub-case cannot meet the absolute 1e-5 in float32: mu = 0 on a tilted normal,
where the force is a n and its three float32 components, and the float32 normal,
each carry half a spacing of rounding -- 1.4e-5 N measured at 390 N, whose
spacing is 3.1e-5 N.  There the bound is max(1e-5, two spacings of |f|); with mu
= 0 on world z, and with mu > 0, the bound stands as it is."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.contact_id_ref import point_jacobians
from tests.contact_qp_ref import DEFAULTS, contact_qp_ref, friction_of, unit_normals
from tests.id_ref import Kinematics, id_ref
from tests.test_contact_id_reference import (CLOSED_LOOP_N, HOLD, HOLD_STEPS, closed_loop_case, feet_contacts)
from tests.test_contact_qp_reference import load_cases
from tests.test_gpu_contact_id import _stance_sim
from tests.test_id_reference import FAR
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd.sim import ContactForces          # (the feature: this file fails without it)

pytestmark = pytest.mark.gpu

N = 8
MODELS = ["thormang", "gogoro"]
ITERS = [1, 8, DEFAULTS["iters"]]
CASES = ["stand", "slope", "share", "toe", "beyond", "lateral", "frictionless", "general"]
# worst max |x - x_ref| / scale per model over every comparison in this file, measured on the MI355X; the tolerance
# is 4 x it
QP_MEASURED = {"thormang": {"force": 2.8e-5, "torque": 2.7e-4}, "gogoro": {"force": 5.0e-5, "torque": 1.7e-4}}
assert 4 * max(v for d in QP_MEASURED.values() for v in d.values()) <= 5e-3
JIT_HASH = 0x7E57_0000_0000_0000


def _setup(name, n, rs):
    """(model, root, dof, contacts, extents) of the test state."""
    from thormang_isaacgym_amd.sim import contact_link_indices, load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_patch
    m = load_model(name)
    D = m.num_dof
    if name == "thormang":
        _desc, _sp, r2, d2, *_ = closed_loop_case(m)
        root, dof = np.repeat(r2[:1], n, axis=0), np.tile(d2[:D], (n, 1))
        dof[:, 0] += rs.uniform(-0.1, 0.1, n * D).astype(np.float32)
        dof[:, 1] = rs.normal(0, 0.5, n * D)
        q = np.array([0.0, 0.0, 0.0, 1.0]) + rs.normal(0, 0.03, (n, 4))
        root[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        root[:, 7:13] = rs.normal(0, 0.2, (n, 6))
        patches = [walk_sole_patch(m, l) for l in walk_feet_indices(m)]
        con = [(int(l), tuple(p[0])) for l, p in zip(walk_feet_indices(m), patches)]
        return m, root, dof, con, [p[1] for p in patches]
    _root, dof = random_state(m, n, rs)
    root = pm.sim(m, n=n)[2]
    root[:, 2] = 0.5
    root[:, 7:13] = rs.normal(0, 0.2, (n, 6))
    a, b = contact_link_indices(m)[:2]
    return m, root, dof, [(int(a), (0.05, 0.0, -0.02)), (int(b), (-0.03, 0.01, 0.04))], [(0.0, 0.0), (0.0, 0.0)]


class Case:
    """A sim of ``n`` envs in the test state with the reference's inputs; ``call`` runs one call, ``check`` compares."""

    def __init__(self, name, n=N, seed=51, fix_base=False, jit=False):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        rs = np.random.default_rng(seed)
        self.name, self.n = name, n
        self.m, self.root, self.dof, self.con, self.ext = m, root, dof, con, ext = _setup(name, n, rs)
        self.D, self.L, self.K = D, L, K = m.num_dof, m.num_bodies, len(con)
        if n > 1:
            root[1, :3] = FAR
        if fix_base:
            root[:, 7:13] = 0.0
        self.ms = rs.uniform(0.8, 1.2, (n, L)).astype(np.float32)
        self.arm = rs.uniform(0.005, 0.02, (n, D)).astype(np.float32)
        ao = dict(fix_base_link=True) if fix_base else {}
        jh = (JIT_HASH | (abi.ModelDesc(m).hash & 0xFFFF_FFFF)) if jit else None
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1, **ao)[1], n, "cuda:0", jit_hash=jh)
        s.root_state.copy_(torch.from_numpy(root))
        s.dof_state.copy_(torch.from_numpy(dof))
        s.set_body_mass_scale_indexed(torch.from_numpy(self.ms).cuda(), torch.arange(n, device="cuda:0"))
        props = abi.default_dof_props(m, n)
        props[abi.TG_PROP_ARMATURE] = self.arm
        s.dof_props.copy_(torch.from_numpy(props))
        s.refresh()
        self.frames = [s.contact_frame(l, off) for l, off in con]
        self.kin = Kinematics(m, root, dof)
        self.cases = load_cases(n, D, K)
        self.tol = {k: 4 * v for k, v in QP_MEASURED[name].items()}
        self.worst = {"force": 0.0, "torque": 0.0}

    def call(self, velocity=True, **kw):
        """dict of numpy outputs of one call; numpy keyword arguments go to the device."""
        dev = {k: (torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda() if isinstance(v, np.ndarray) else v)
               for k, v in kw.items()}
        for t in getattr(self.s, "_qp_out", {}).values():
            t.fill_(float("nan"))
        got = self.s.contact_qp(self.frames, self.ext, velocity=velocity, forces=True, info=True, **dev)
        assert isinstance(got, ContactForces)
        torch.cuda.synchronize()
        return {k: getattr(got, k).cpu().numpy().copy() for k in ContactForces._fields}

    def reference(self, velocity=True, **kw):
        kw = {k: v for k, v in kw.items() if k not in ("efforts", "dofs", "accumulate")}
        return contact_qp_ref(self.m, self.root, self.dof, self.con, self.ext, velocity=velocity, mass_scale=self.ms,
                              armature=self.arm, kin=self.kin, **kw)

    def feasible(self, got, kw):
        """every returned force is in its cone: on the device's own output, with the float64 unit normals"""
        nrm = unit_normals(kw.get("normals"), self.n, self.K)[:, :, None, :]
        mu = friction_of(kw.get("mu", 0.7), kw.get("friction"), self.n, self.K)[:, :, None]
        f = got["forces"].astype(np.float64)
        fn = (f * nrm).sum(-1)
        ft = np.linalg.norm(f - fn[..., None] * nrm, axis=-1)
        assert (fn >= 0.0).all(), fn.min()
        # (mu = 0 on a tilted normal: a float32 force cannot lie nearer the normal's line than the rounding of its
        # components and of the float32 normal allows, two spacings of |f|; see the module's docstring)
        slack = np.where(mu == 0, 2 * np.spacing(np.abs(got["forces"]).max(axis=-1)).astype(np.float64), 0.0)
        assert (ft <= mu * fn * (1 + 1e-5) + np.maximum(1e-5, slack)).all(), float((ft - mu * fn).max())

    def check(self, got, ref, what, kw=None):
        n, K, D = self.n, self.K, self.D
        for k, shape in (("tau", (n, 6 + D)), ("wrench", (n, K, 6)), ("forces", (n, K, 4, 3)), ("info", (n, 4))):
            assert got[k].shape == shape and got[k].dtype == np.float32 and not np.isnan(got[k]).any(), k
        b = ref["b"]
        Fs, Ts = float(np.abs(b[:, :3]).max()), float(np.abs(b[:, 3:]).max())
        d = lambda a, r: float(np.abs(a - r).max())
        fig = {"model": self.name, "what": what,
               "forces": d(got["forces"], ref["forces"]) / Fs, "wrench_f": d(got["wrench"][..., :3], ref["wrench"][..., :3]) / Fs,
               "wrench_n": d(got["wrench"][..., 3:], ref["wrench"][..., 3:]) / Ts,
               "base_f": d(got["tau"][:, :3], ref["tau"][:, :3]) / Fs, "base_n": d(got["tau"][:, 3:6], ref["tau"][:, 3:6]) / Ts,
               "tau": d(got["tau"][:, 6:], ref["tau"][:, 6:]) / Ts, "info_f": d(got["info"][:, 0], ref["info"][:, 0]) / Fs,
               "info_n": d(got["info"][:, 1], ref["info"][:, 1]) / Ts, "max_force": Fs, "max_torque": Ts}
        fig["force"] = max(fig[k] for k in ("forces", "wrench_f", "base_f", "info_f"))
        fig["torque"] = max(fig[k] for k in ("wrench_n", "base_n", "tau", "info_n"))
        if n > 1:
            fig["far_forces"] = d(got["forces"][1], ref["forces"][1]) / Fs
        # the loaded vertices: a difference only where the reference's normal force is within the tolerance of 0
        nrm = unit_normals((kw or {}).get("normals"), n, K)[:, :, None, :]
        fn = (ref["forces"] * nrm).sum(-1).reshape(n, -1)
        near = (np.abs(fn) <= self.tol["force"] * Fs).sum(axis=1)
        off = np.abs(got["info"][:, 3] - ref["info"][:, 3])
        fig["count_off"] = int(off.sum())
        for k in ("force", "torque"):
            self.worst[k] = max(self.worst[k], fig[k])
        print(fig)
        assert fig["force"] <= self.tol["force"] and fig["torque"] <= self.tol["torque"], fig
        assert (off <= near).all() and off.sum() <= 0.02 * fn.size, fig
        assert (got["info"][:, 2] >= 0).all()
        if kw is not None:
            self.feasible(got, kw)
        return fig


_cases = {}


def shared(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", MODELS)
def test_parity_with_the_reference_at_the_same_iteration_count(name, case, iters):
    """The load cases of the convergence trial after 1, 8 and the default number of iterations: forces, wrench, tau
    and info against the float64 reference after as many; every returned force in its cone."""
    c = shared(name)
    kw = dict(c.cases[case], iters=iters)
    got, ref = c.call(**kw), c.reference(**kw)
    c.check(got, ref, f"{case}, {iters} iterations", kw)
    assert np.abs(ref["forces"]).max() > 1.0
    if iters == DEFAULTS["iters"]:
        # float32 rounding alone (the reference's iteration in float32) moves no more loaded-vertex counts than allowed
        r32 = c.reference(dtype=np.float32, **kw)
        assert np.abs(r32["info"][:, 3] - ref["info"][:, 3]).sum() <= 0.02 * 4 * c.K * c.n


@pytest.mark.parametrize("share", ["none", "mixed", "zero"])
@pytest.mark.parametrize("mu", ["zero", "0.3", "tensor"])
@pytest.mark.parametrize("name", MODELS)
def test_friction_and_shares(name, mu, share):
    """mu 0, 0.3 and a per-env tensor (with a negative and a NaN entry, taken as 0) against shares None, mixed with
    a zero, and all zero, on a general acceleration over tilted normals, after 1 and the default iterations: a zero
    share gives exact zeros, an env with every share 0 the plain inverse dynamics of the device."""
    c = shared(name)
    rs = np.random.default_rng(7)
    kw = dict(accel=c.cases["general"]["accel"], normals=c.cases["slope"]["normals"])
    if mu == "tensor":
        fr = rs.uniform(0.1, 0.9, (c.n, c.K)).astype(np.float32)
        fr[2, 0], fr[3, c.K - 1] = -0.5, np.nan
        kw["friction"] = fr
    else:
        kw["mu"] = 0.0 if mu == "zero" else 0.3
    sh = None
    if share != "none":
        sh = rs.uniform(0.2, 1.0, (c.n, c.K)).astype(np.float32)
        sh[0, 0], sh[2, c.K - 1], sh[4, 0], sh[3] = 0.0, 0.0, -0.7, 0.0
        if share == "zero":
            sh[:] = 0.0
        kw["share"] = sh
    for iters in (1, DEFAULTS["iters"]):
        got, ref = c.call(iters=iters, **kw), c.reference(iters=iters, **kw)
        c.check(got, ref, f"mu {mu}, share {share}, {iters} iterations", kw)
        if sh is not None:
            zero = ~(sh > 0)
            assert (got["forces"][zero] == 0.0).all() and (got["wrench"][zero] == 0.0).all()
            out = torch.full((c.n, 6 + c.D), float("nan"), dtype=torch.float32, device="cuda:0")
            c.s.inverse_dynamics(accel=torch.from_numpy(kw["accel"]).cuda(), out=out)
            torch.cuda.synchronize()
            air = zero.all(axis=1)
            assert air.any()
            d = np.abs(got["tau"][air] - out.cpu().numpy()[air]).max() / np.abs(ref["b"]).max()
            assert d <= c.tol["torque"] and (got["info"][air, 2:] == 0.0).all()
    if share == "mixed":
        # env 0 without its contact 0 equals the call without that contact
        keep = list(range(1, c.K))
        k2 = dict(kw, share=sh[:, keep], normals=kw["normals"][:, keep])
        if "friction" in k2:
            k2["friction"] = kw["friction"][:, keep]
        one = contact_qp_ref(c.m, c.root, c.dof, [c.con[i] for i in keep], [c.ext[i] for i in keep], mass_scale=c.ms,
                             armature=c.arm, kin=c.kin, **k2)
        Fs, Ts = np.abs(ref["b"][:, :3]).max(), np.abs(ref["b"][:, 3:]).max()
        assert np.abs(got["forces"][0, keep] - one["forces"][0]).max() <= c.tol["force"] * Fs
        assert np.abs(got["tau"][0, 6:] - one["tau"][0, 6:]).max() <= c.tol["torque"] * Ts


@pytest.mark.parametrize("name", MODELS)
def test_identity_with_the_sibling(name):
    """With wrench from this call, tau[6:] equals b[6:] - sum_k Jp_k^T wrench_k formed on the host in float64 from
    jacobian_ref's rows and id_ref's b, within the tolerance."""
    c = shared(name)
    kw = c.cases["general"]
    got = c.call(**kw)
    b = id_ref(c.m, c.root, c.dof, accel=kw["accel"], mass_scale=c.ms, armature=c.arm, kin=c.kin)
    Jp = point_jacobians(c.kin, c.con)
    tau = b.copy()
    for e in range(c.n):
        for i in range(c.K):
            tau[e] -= Jp[e, i].T @ got["wrench"][e, i].astype(np.float64)
    d = np.abs(got["tau"] - tau).max() / np.abs(b[:, 3:]).max()
    print({"model": name, "identity_with_the_sibling": float(d)})
    assert d <= c.tol["torque"]


def test_interior_case_is_close_to_the_least_squares_call():
    """The CPU file's interior case (the stance, standing, flat, mu 0.7) on the device: tau[6:] is within reg f_max /
    F of Sim.contact_inverse_dynamics's at equal shares on the CPU test's scale for moments, F r_max (the reg bound
    of tests/test_contact_qp_reference.py: the wrench moments differ by that much, and the ankles carry them).
    Measured 3.0e-3 against 4.8e-3 (1.1 N m, 0.14 of the largest joint torque of the standing robot)."""
    from thormang_isaacgym_amd.sim import Sim, load_model
    from tests.contact_qp_ref import patch_vertices
    from tests.test_contact_qp_reference import stance
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    m, root, dof, con, ext, kin = stance()
    rmax = np.linalg.norm(patch_vertices(kin, con, ext)[1] - kin.c[:, None, None, 0], axis=-1).max()
    s = Sim(m, pm.sim(m, n=2, dt=0.01, substeps=1)[1], 2, "cuda:0")
    s.root_state.copy_(torch.from_numpy(root))
    s.dof_state.copy_(torch.from_numpy(dof))
    frames = [s.contact_frame(l, off) for l, off in con]
    qp = s.contact_qp(frames, ext, mu=0.7, velocity=False, forces=True)
    ls = s.contact_inverse_dynamics(frames, velocity=False)
    torch.cuda.synchronize()
    f = qp.forces.cpu().numpy().astype(np.float64)
    F = np.linalg.norm(qp.wrench.cpu().numpy()[:, :, :3].sum(axis=1), axis=-1).min()
    bound = DEFAULTS["reg"] * np.linalg.norm(f, axis=-1).max() / F
    a, b = qp.tau.cpu().numpy()[:, 6:], ls.tau.cpu().numpy()[:, 6:]
    fig = {"tau_rel": float(np.abs(a - b).max() / (F * rmax)), "bound": float(bound),
           "of_the_largest_torque": float(np.abs(a - b).max() / np.abs(b).max())}
    print(fig)
    assert fig["tau_rel"] <= bound, fig


@pytest.mark.parametrize("name", MODELS)
def test_runtime_loaded_model_equals_compiled_in(name):
    """The model registered under another hash runs the hipRTC build of the kernel: max |compiled-in - run-time| is
    what the sibling kernel measured (tests/test_gpu_physics.py ON_DEMAND_MEASURED: 0), floored at one spacing of
    the output's largest value as there."""
    a, b = shared(name), Case(name, jit=True)
    assert not a.s.jit and b.s.jit
    kw = a.cases["lateral"]
    x, y = a.call(**kw), b.call(**kw)
    for k in x:
        top = float(np.abs(x[k]).max())
        diff = float(np.abs(x[k] - y[k]).max())
        print({"model": name, "output": k, "compiled_vs_runtime": diff})
        assert top > 0 and diff <= float(np.spacing(np.float32(top))), (k, diff)


@pytest.mark.parametrize("name", MODELS)
def test_state_is_unchanged_and_calls_repeat_bit_for_bit(name):
    c = shared(name)
    s = c.s
    keep = [t.clone() for t in (s.root_state, s.dof_state, s.dof_props, s.dof_actuation, s.dof_pos_target,
                                s.dof_vel_target)]
    kw = c.cases["slope"]
    a, b = c.call(**kw), c.call(**kw)
    assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)
    now = (s.root_state, s.dof_state, s.dof_props, s.dof_actuation, s.dof_pos_target, s.dof_vel_target)
    assert all(torch.equal(x, y) for x, y in zip(keep, now))
    assert np.array_equal(s.root_state.cpu().numpy(), c.root) and np.array_equal(s.dof_state.cpu().numpy(), c.dof)
    # without forces / info the parts are None and tau, wrench keep their bits
    only = s.contact_qp(c.frames, c.ext, mu=kw["mu"], normals=torch.from_numpy(kw["normals"]).cuda())
    torch.cuda.synchronize()
    assert only.forces is None and only.info is None
    assert np.array_equal(only.tau.cpu().numpy(), a["tau"]) and np.array_equal(only.wrench.cpu().numpy(), a["wrench"])


def test_the_far_env_gets_the_same_bits():
    """An env copied to (300, -200, 1) gives bit-identical outputs."""
    c = Case("thormang", n=2, seed=53)
    s = c.s
    root = c.root.copy()
    root[1] = root[0]
    root[1, :3] = FAR
    s.root_state.copy_(torch.from_numpy(root))
    s.dof_state.reshape(2, c.D, 2)[1] = s.dof_state.reshape(2, c.D, 2)[0]
    s.set_body_mass_scale_indexed(torch.from_numpy(np.stack([c.ms[0], c.ms[0]])).cuda(), torch.arange(2, device="cuda:0"))
    s.dof_props[:, 1] = s.dof_props[:, 0]
    s.refresh()
    got = c.call(**c.cases["lateral"])
    for k, v in got.items():
        assert np.array_equal(v[0], v[1]), k
    assert np.abs(got["forces"]).max() > 1.0


@pytest.mark.parametrize("name", MODELS)
def test_one_env(name):
    c = Case(name, n=1, seed=52)
    kw = c.cases["general"]
    c.check(c.call(**kw), c.reference(**kw), "one env", kw)


def test_fix_base_writes_the_full_layout():
    c = Case("thormang", fix_base=True)
    assert c.s.params.fix_base
    kw = c.cases["general"]
    c.check(c.call(**kw), c.reference(**kw), "fix_base", kw)


def test_efforts():
    """The clamp at a deliberately small effort limit, DOF selection, a sentinel in every element that is not
    selected, and accumulate, as the sibling's test."""
    c = Case("thormang")
    s, D, n = c.s, c.D, c.n
    names = ["l_leg_kn_p", "r_leg_hip_p", "l_leg_an_r", "l_arm_sh_p1", "torso_y"]
    idx = [c.m.dof_names.index(x) for x in names]
    kw = c.cases["stand"]
    ref = c.reference(**kw)["tau"]
    low = idx[int(np.argmax(np.abs(ref[:, [6 + d for d in idx]]).min(axis=0)))]
    lim = np.float32(0.5 * np.abs(ref[:, 6 + low]).min())
    assert lim > 1e-3
    s.dof_props[abi.TG_PROP_EFFORT][:, low] = float(lim)
    s.refresh()
    effort = s.dof_props[abi.TG_PROP_EFFORT].cpu().numpy()
    sentinel = torch.arange(n * D, dtype=torch.float32, device="cuda:0").reshape(n, D) * 0.5 + 1000.0
    sel = np.zeros(D, bool)
    sel[idx] = True
    eff = sentinel.clone()
    tau = c.call(dofs=names, efforts=eff, **kw)["tau"]
    got = eff.cpu().numpy()
    assert np.array_equal(got[:, ~sel], sentinel.cpu().numpy()[:, ~sel])
    assert np.array_equal(got[:, sel], np.clip(tau[:, 6:], -effort, effort)[:, sel])
    assert set(np.abs(got[:, low]).tolist()) == {float(lim)}                 # the clamp acts in every env
    eff2 = sentinel.clone()
    c.call(dofs=idx, efforts=eff2, **kw)
    assert torch.equal(eff2, eff)                                            # by index: the same
    base = (torch.arange(n * D, dtype=torch.float32, device="cuda:0").reshape(n, D) % 7 - 3.0) * 0.25
    eff3 = base.clone()
    c.call(dofs=idx, efforts=eff3, accumulate=True, **kw)
    got3, b0 = eff3.cpu().numpy(), base.cpu().numpy()
    assert np.array_equal(got3[:, ~sel], b0[:, ~sel])
    np.testing.assert_allclose(got3[:, sel], np.clip(b0 + tau[:, 6:], -effort, effort)[:, sel], rtol=1e-6, atol=1e-7)
    assert (np.abs(got3[:, low]) <= lim).all()
    # every DOF, efforts alone through the C ABI
    from thormang_isaacgym_amd._lib import lib
    eff4 = sentinel.clone()
    frames = (abi.tg_contact_frame * c.K)(*c.frames)
    hxy = (C.c_float * (2 * c.K))(*[v for x in c.ext for v in x])
    d = DEFAULTS
    assert lib().tg_contact_qp(s.handle, frames, c.K, hxy, None, None, kw["mu"], None, 0.1, d["reg"], d["rho"],
                               d["relax"], d["iters"], 3, None, None, None, None, None, eff4.data_ptr(), None, 0,
                               0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(eff4.cpu().numpy(), np.clip(tau[:, 6:], -effort, effort))


def test_measured_figures_are_on_record():
    """The worst figures of this run, printed for QP_MEASURED (run last: the shared cases have made their calls)."""
    for name, c in _cases.items():
        print({"model": name, "worst": c.worst, "measured": QP_MEASURED[name]})
        assert all(c.worst[k] <= 4 * QP_MEASURED[name][k] for k in c.worst)


# ---------------------------------------------------------------- closed loop on the device
def _feet(s, m):
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_patch
    patches = [walk_sole_patch(m, l) for l in walk_feet_indices(m)]
    return [s.contact_frame(l, p[0]) for l, p in zip(walk_feet_indices(m), patches)], [p[1] for p in patches]


def test_closed_loop_holds_the_standing_robot():
    """The standing test of tests/test_gpu_contact_id.py with contact_qp(..., efforts=dof_actuation) in place of the
    sibling: the posture is held within the same HOLD bound.  The balance is soft, so the torques assume a base
    wrench that is off by the effect of reg, and a robot that balances without feedback amplifies that: with the
    default reg 0.03 the drift is 0.151 rad (measured, on the device and with the fp64 oracle loop alike), with 0.01
    0.057, with the 0.003 used here 0.019; an interior case like this one converges in 64 iterations at rho 0.1."""
    s, dof0, m = _stance_sim()
    feet, ext = _feet(s, m)
    for _ in range(HOLD_STEPS):
        s.contact_qp(feet, ext, reg=0.003, rho=0.1, efforts=s.dof_actuation)
        s.simulate()
    torch.cuda.synchronize()
    held = s.dof_state.cpu().numpy().reshape(-1, 2)
    fig = {"held": float(np.abs(held[:, 0] - dof0[:, 0]).max()), "bound": HOLD}
    print(fig)
    assert np.isfinite(held).all() and fig["held"] <= HOLD, fig


def test_closed_loop_push_keeps_the_predicted_forces_in_the_cone():
    """4 envs (2 x the stance), a 150 N lateral push on the pelvis, mu 0.2: this call's predicted wrenches keep
    |f_xy| <= mu f_z in every step, the sibling's in the same states do not."""
    from thormang_isaacgym_amd.sim import Sim, load_model
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from tests.test_contact_id_reference import SETTLE_STEPS, effort_mode
    m = load_model("thormang")
    n, mu = 4, 0.2
    _desc, _sp2, root, dof, props, pt, _vt = closed_loop_case(m)
    sp = pm.sim(m, n=n, dt=1.0 / 120.0, substeps=1)[1]
    s = Sim(m, sp, n, "cuda:0")
    tile = lambda a, ax=0: np.concatenate([a, a], axis=ax)
    s.root_state.copy_(torch.from_numpy(tile(root)))
    s.dof_state.copy_(torch.from_numpy(tile(dof)))
    s.dof_props.copy_(torch.from_numpy(tile(props, 1)))
    s.dof_pos_target.copy_(torch.from_numpy(tile(pt)))
    s.dof_actuation.zero_()
    s.refresh()
    for _ in range(SETTLE_STEPS):
        s.simulate()
    s.dof_props.copy_(torch.from_numpy(effort_mode(tile(props, 1))))
    s.refresh()
    feet, ext = _feet(s, m)
    push = torch.zeros(n, s.L, 3, dtype=torch.float32, device="cuda:0")
    push[:, 0, 1] = 150.0
    # the push as the controller knows it: an acceleration demand on the base that the feet would have to supply
    mass = float(np.asarray(abi.model_arrays(m)["link_inertia"], np.float64)[:, 0].sum())
    accel = torch.zeros(n, 6 + s.D, dtype=torch.float32, device="cuda:0")
    accel[:, 1] = -150.0 / mass
    worst_qp, worst_ls = 0.0, 0.0
    for _ in range(20):
        ls = s.contact_inverse_dynamics(feet, accel=accel).wrench.clone()
        qp = s.contact_qp(feet, ext, mu=mu, accel=accel, efforts=s.dof_actuation).wrench.clone()
        s.apply_rigid_body_force_tensors(push)
        s.simulate()
        for w, key in ((qp, "qp"), (ls, "ls")):
            ratio = float((w[:, :, :2].norm(dim=-1) - mu * w[:, :, 2]).max())
            if key == "qp":
                worst_qp = max(worst_qp, ratio)
            else:
                worst_ls = max(worst_ls, ratio)
    torch.cuda.synchronize()
    fig = {"qp_max_fxy_minus_mu_fz": worst_qp, "sibling_max_fxy_minus_mu_fz": worst_ls}
    print(fig)
    assert torch.isfinite(s.dof_state).all()
    assert worst_qp <= 1e-3 and worst_ls > 10.0, fig
