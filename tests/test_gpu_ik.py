"""Damped-least-squares IK on the GPU (tg_ik_dls, Sim.ik_chain / Sim.solve_ik)
against the float64 reference built from the oracle (tests/ik_ref.py).

Five envs (no multiple of anything), env 1 far out on the grid at
(300, -200, 1), random states, goals = the link poses at perturbed joint angles
plus noise (the goal quaternions are not unit: the kernel normalises them),
the output tensors filled with NaN before each call.

Tolerance for dq (rad, m) and err (m, quaternion units): max |x - x_ref| <=
4 x the worst value measured on the MI355X over the calls these tests make
(IK_MEASURED below), hard cap 1e-4.  Measured: thormang dq 2.7e-7 / err
2.8e-7, gogoro 5.4e-7 / 4.8e-7, the run-time jit_walker 1.3e-7 / 1.2e-7, the
far env no worse than the others (1.5e-7 / 0.9e-7 on thormang).  The float32
evaluation of the reference formula itself differs from float64 by 1.2e-7 at
lambda = 0.3 (cond ~ 40); the rest is the float32 forward kinematics with the
hardware sine and cosine.  A centre-of-mass point instead of the link origin
changes dq by 1.6e-2 rad on l_leg_foot_link in these states, a dropped column
or a wrong sign by as much or more."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests.ik_ref import chain_spec, ik_ref, link_pose_goal, pose_error
from tests.test_ik_reference import CONVERGENCE_CASES, FAR, convergence_case, error_norms
from tests.test_rigid_body_states import random_state
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

N = 5
LAMBDA = 0.3
# worst max |dq - dq_ref| and max |err - err_ref| per model, measured on the MI355X
# over every comparison in this file; the tolerance is 4 x it, hard cap 1e-4
IK_MEASURED = {"thormang": {"dq": 2.8e-7, "err": 2.9e-7}, "gogoro": {"dq": 5.4e-7, "err": 4.8e-7},
               "jit_walker": {"dq": 1.4e-7, "err": 1.2e-7}}
assert 4 * max(max(v.values()) for v in IK_MEASURED.values()) <= 1e-4


def _model(name):
    from thormang_isaacgym_amd.sim import load_model
    return pm.jit_walker() if name == "jit_walker" else load_model(name)


def chains_for(name, s):
    """the chains of a model's test, built through Sim.ik_chain (names and indices)"""
    if name == "thormang":
        return [s.ik_chain("l_arm_end_link"),                                   # 8 DOFs, torso_y included
                s.ik_chain("r_arm_end_link", num_dofs=8),
                s.ik_chain("l_leg_foot_link"),                                   # 6 DOFs, com off the origin
                s.ik_chain("r_leg_foot_link", num_dofs=6, offset=(0.05, -0.02, -0.03))]
    if name == "gogoro":
        left = s.ik_chain("l_arm_end_link", num_dofs=7)                          # the reference's 7 arm columns, all locked
        right = s.ik_chain("r_arm_end_link", dofs=["base_y", "r_arm_sh_p1", "r_arm_sh_r", "r_arm_sh_p2", "r_arm_el_y",
                                                   "r_arm_wr_r", "r_arm_wr_y", "r_arm_wr_p"])   # a prismatic locked column
        d = [int(left.dofs[i]) for i in range(7)]
        off_path = s.ik_chain("l_arm_end_link", dofs=d[:3] + [s.model.dof_names.index("r_arm_sh_p1")] + d[3:])
        return [left, right, off_path]
    return [s.ik_chain("l_shin", offset=(0.0, 0.0, -0.26)), s.ik_chain(4, dofs=[2, 3], offset=(0.0, 0.01, -0.26))]


class Case:
    """A sim of ``n`` envs in the test state with its chains, goals and the
    reference; ``call`` runs one solve on NaN-filled outputs."""

    def __init__(self, name, n=N, seed=23):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.name, self.m, self.n = name, _model(name), n
        m = self.m
        self.D, self.L = m.num_dof, m.num_bodies
        rs = np.random.default_rng(seed)
        self.root, self.dof = random_state(m, n, rs)
        if n > 1:
            self.root[1, :3] = FAR
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        self.chains = chains_for(name, s)
        self.K = K = len(self.chains)
        moved = self.dof.reshape(n, self.D, 2).copy()
        moved[:, :, 0] += rs.uniform(-0.25, 0.25, (n, self.D)).astype(np.float32)
        moved = np.ascontiguousarray(moved.reshape(n * self.D, 2))
        gp, gq = np.zeros((n, K, 3), np.float32), np.zeros((n, K, 4), np.float32)
        for k, ch in enumerate(self.chains):
            p, q = link_pose_goal(m, self.root, moved, ch)
            gp[:, k] = p + rs.normal(0, 0.01, (n, 3)).astype(np.float32)
            gq[:, k] = (q + rs.normal(0, 0.02, (n, 4))) * rs.uniform(0.5, 2.0, (n, 1))
        if name == "gogoro":                                                # chain 2 is chain 0 plus an off-path DOF: the same goal
            gp[:, 2], gq[:, 2] = gp[:, 0], gq[:, 0]
        self.gp, self.gq = gp, gq
        self.gp_t, self.gq_t = torch.from_numpy(gp).cuda(), torch.from_numpy(gq).cuda()
        self.tol = {k: 4 * v for k, v in IK_MEASURED[name].items()}

    def call(self, orient=True, targets=None):
        s = self.s
        gq = self.gq_t if orient else None
        s.solve_ik(self.chains, self.gp_t, gq, damping=LAMBDA)           # (allocates the outputs on first use)
        for t in s._ik_out[self.K]:
            t.fill_(float("nan"))
        dq, err = s.solve_ik(self.chains, self.gp_t, gq, damping=LAMBDA, targets=targets, return_error=True)
        torch.cuda.synchronize()
        return dq.cpu().numpy(), err.cpu().numpy()

    def reference(self, orient=True):
        return ik_ref(self.m, self.root, self.dof, self.chains, self.gp, self.gq if orient else None, LAMBDA)

    def check(self, got, ref, what):
        dq, err = got
        dq_ref, err_ref = ref
        assert dq.shape == (self.n, self.K, 8) and err.shape == (self.n, self.K, 6)
        assert not np.isnan(dq).any() and not np.isnan(err).any()
        for k, ch in enumerate(self.chains):
            assert (dq[:, k, ch.num_dofs:] == 0.0).all()                  # the padding, exactly
        fig = {"model": self.name, "what": what, "dq_err": float(np.abs(dq - dq_ref).max()),
               "err_err": float(np.abs(err - err_ref).max()), "max_abs_dq": float(np.abs(dq_ref).max()),
               "max_abs_err": float(np.abs(err_ref).max())}
        if self.n > 1:
            others = [e for e in range(self.n) if e != 1]
            fig["far_env"] = (float(np.abs(dq[1] - dq_ref[1]).max()), float(np.abs(err[1] - err_ref[1]).max()))
            fig["other_envs"] = (float(np.abs(dq[others] - dq_ref[others]).max()),
                                 float(np.abs(err[others] - err_ref[others]).max()))
        print(fig)
        assert fig["dq_err"] <= self.tol["dq"], fig
        assert fig["err_err"] <= self.tol["err"], fig


_cases = {}


def shared(name):
    """One shared Case per model with both calls made and both references computed, read-only."""
    if name not in _cases:
        c = Case(name)
        c.got6, c.got3 = c.call(True), c.call(False)
        c.ref6, c.ref3 = c.reference(True), c.reference(False)
        _cases[name] = c
    return _cases[name]


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_pose_rows_match_the_reference(name):
    c = shared(name)
    c.check(c.got6, c.ref6, "6 rows")


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_position_only_matches_the_reference(name):
    c = shared(name)
    c.check(c.got3, c.ref3, "3 rows")
    assert (c.got3[1][..., 3:] == 0.0).all()                              # err[3:6] written as 0
    assert np.abs(c.got3[0] - c.got6[0]).max() > 1e-3                      # (the two systems differ)


def test_the_origin_convention_shows_on_the_foot_chains():
    """l_leg_foot_link's com is off its origin and r_leg_foot_link carries an
    offset: a reference with the wrong controlled point is far outside the tolerance."""
    c = shared("thormang")
    a = abi.model_arrays(c.m)
    wrong = []
    for ch in c.chains:
        link, dofs, offset = chain_spec(ch)
        wrong.append((link, dofs, [float(v) for v in a["link_inertia"][link, 1:4]]))   # the com as the point
    dq_w, err_w = ik_ref(c.m, c.root, c.dof, wrong, c.gp, c.gq, LAMBDA)
    for k in (2, 3):
        d = float(np.abs(dq_w[:, k] - c.ref6[0][:, k]).max())
        print({"chain": k, "dq_change_with_the_com_as_point": d})
        assert d > 10 * c.tol["dq"]
    assert any(np.linalg.norm(a["link_inertia"][chain_spec(ch)[0], 1:4]) > 1e-2 for ch in c.chains)
    assert any(np.linalg.norm(chain_spec(ch)[2]) > 0 for ch in c.chains)


def test_off_path_column_is_exactly_zero():
    """gogoro chain 2 = chain 0 with r_arm_sh_p1 (off l_arm_end_link's path) as its column 3."""
    c = shared("gogoro")
    for dq in (c.got6[0], c.got3[0]):
        assert (dq[:, 2, 3] == 0.0).all()
        rest = np.delete(dq[:, 2, :8], 3, axis=1)
        np.testing.assert_allclose(rest, c.ref6[0][:, 0, :7] if dq is c.got6[0] else c.ref3[0][:, 0, :7], rtol=0,
                                   atol=c.tol["dq"])
        assert np.abs(rest).max() > 1e-3
    assert (c.ref6[0][:, 2, 3] == 0.0).all()                               # (the reference agrees: a zero column)


def test_locked_and_prismatic_columns_move():
    """gogoro: every arm DOF is locked, and chain 1 carries the prismatic locked base_y: ordinary columns."""
    c = shared("gogoro")
    assert set(chain_spec(c.chains[0])[1]) <= set(c.m.locked_dofs)
    assert c.m.dof_names[chain_spec(c.chains[1])[1][0]] == "base_y"
    assert (np.abs(c.got6[0][:, 0, :7]).max(axis=0) > 1e-4).all()
    assert (np.abs(c.got6[0][:, 1, 0]) > 1e-4).any()


def test_runtime_loaded_model():
    """A model compiled at run time (tg_model_jit): the call works, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = shared("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()
    c.check(c.got6, c.ref6, "6 rows")
    c.check(c.got3, c.ref3, "3 rows")


def test_position_targets():
    """A sentinel-filled [N, D] tensor keeps every non-chain element bit for
    bit; chain DOFs are q + the sum of the returned dq; the shared torso_y
    gets both arms' steps."""
    c = Case("thormang")
    sentinel = (torch.arange(N * c.D, dtype=torch.float32, device="cuda:0").reshape(N, c.D) * 0.5 + 1000.0)
    tg = sentinel.clone()
    dq, _err = c.call(True, targets=tg)
    got = tg.cpu().numpy()
    q = c.dof.reshape(N, c.D, 2)[:, :, 0]
    expect, touched = sentinel.cpu().numpy().copy(), np.zeros(c.D, bool)
    total = np.zeros((N, c.D), np.float32)
    for k, ch in enumerate(c.chains):                                     # ascending (k, c), float32 as the kernel sums
        for i in range(ch.num_dofs):
            total[:, ch.dofs[i]] += dq[:, k, i]
            touched[ch.dofs[i]] = True
    expect[:, touched] = (q + total)[:, touched]
    assert touched.sum() == 8 + 7 + 6 + 6 and touched.sum() < c.D
    assert np.array_equal(got[:, ~touched], sentinel.cpu().numpy()[:, ~touched])
    np.testing.assert_allclose(got[:, touched], expect[:, touched], rtol=0, atol=1e-6)
    torso = c.m.dof_names.index("torso_y")
    assert c.chains[0].dofs[0] == torso and c.chains[1].dofs[0] == torso
    np.testing.assert_allclose(got[:, torso], q[:, torso] + (dq[:, 0, 0] + dq[:, 1, 0]), rtol=0, atol=1e-6)
    assert (np.abs(dq[:, 0, 0]) > 1e-4).all() and (np.abs(dq[:, 1, 0]) > 1e-4).all()
    # targets alone (no dq, no err) through the C ABI: the same result
    from thormang_isaacgym_amd._lib import lib
    tg2 = sentinel.clone()
    arr = (abi.tg_ik_chain * c.K)(*c.chains)
    assert lib().tg_ik_dls(c.s.handle, arr, c.K, c.gp_t.data_ptr(), c.gq_t.data_ptr(), LAMBDA, None, None,
                           tg2.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(tg2, tg)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_state_is_unchanged(name):
    c = shared(name)
    s = c.s
    root0, dof0 = s.root_state.clone(), s.dof_state.clone()
    tg = torch.zeros(N, c.D, dtype=torch.float32, device="cuda:0")
    s.solve_ik(c.chains, c.gp_t, c.gq_t, damping=LAMBDA, targets=tg)
    torch.cuda.synchronize()
    assert torch.equal(s.root_state, root0) and torch.equal(s.dof_state, dof0)
    assert np.array_equal(root0.cpu().numpy(), c.root) and np.array_equal(dof0.cpu().numpy(), c.dof)


@pytest.mark.parametrize("link_name,seed", CONVERGENCE_CASES)
def test_iterations_converge_on_the_device(link_name, seed):
    """The reference test's setup and condition (tests/test_ik_reference.py): 20
    calls with set_dof_state_indexed between them bring both error norms to
    <= 10 % of their initial value in every env, judged by the reference's
    pose error at the device's final state."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from thormang_isaacgym_amd.sim import Sim, load_model
    m = load_model("thormang")
    n, D = 3, m.num_dof
    root, dof, chain, gp, gq = convergence_case(m, link_name, seed, n)
    s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
    s.root_state.copy_(torch.from_numpy(root))
    s.dof_state.copy_(torch.from_numpy(dof))
    ch = s.ik_chain(link_name)
    assert chain_spec(ch)[:2] == (chain[0], chain[1])
    nd = ch.num_dofs
    idx = torch.tensor(chain[1], dtype=torch.long, device="cuda:0")
    gp_t, gq_t = torch.from_numpy(gp[:, None].copy()).cuda(), torch.from_numpy(gq[:, None].copy()).cuda()
    p0, o0 = error_norms(pose_error(m, root, dof, chain, gp, gq))
    for _ in range(20):
        dq = s.solve_ik([ch], gp_t, gq_t, damping=LAMBDA)
        new = s.dof_state.clone()
        new.view(n, D, 2)[:, idx, 0] += dq[:, 0, :nd]
        s.set_dof_state_indexed(new, s.all_ids)
    _dq, err = s.solve_ik([ch], gp_t, gq_t, damping=LAMBDA, return_error=True)
    torch.cuda.synchronize()
    final = s.dof_state.cpu().numpy()
    p1, o1 = error_norms(pose_error(m, root, final, chain, gp, gq))
    pd, od = error_norms(err[:, 0].cpu().numpy())
    print({"link": link_name, "pos": (float(p0.max()), float(p1.max())), "orn": (float(o0.max()), float(o1.max())),
           "worst_ratio": (float((p1 / p0).max()), float((o1 / o0).max())),
           "device_err_norms": (float(pd.max()), float(od.max()))})
    assert (p1 <= 0.10 * p0).all() and (o1 <= 0.10 * o0).all(), (p0, p1, o0, o1)
    assert (pd <= 0.10 * p0).all() and (od <= 0.10 * o0).all(), (p0, pd, o0, od)


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_one_env(name):
    c = Case(name, n=1)
    c.check(c.call(True), c.reference(True), "one env")


def test_argument_errors():
    """Every argument error of the header returns TG_ERR_ARG with tg_ik_dls in the message."""
    from thormang_isaacgym_amd._lib import lib
    c = shared("thormang")
    s, L = c.s, lib()
    good = c.chains[0]
    dq = torch.zeros(N, 8, 8, device="cuda:0")
    gp = torch.zeros(N, 8, 3, device="cuda:0")

    def call(chains=(good,), num=None, goal=gp.data_ptr(), damping=LAMBDA, out=dq.data_ptr(), null_chains=False):
        arr = None if null_chains else (abi.tg_ik_chain * max(len(chains), 1))(*chains)
        rc = L.tg_ik_dls(s.handle, arr, len(chains) if num is None else num, goal, None, damping, out, None, None)
        return rc, L.tg_last_error()

    def edited(**kw):
        ch = abi.tg_ik_chain.from_buffer_copy(good)
        for k, v in kw.items():
            if k == "dofs":
                for i, x in enumerate(v):
                    ch.dofs[i] = x
            else:
                setattr(ch, k, v)
        return ch

    assert call()[0] == 0
    bad = {
        "null chains": dict(null_chains=True, num=1),
        "null goal_pos": dict(goal=None),
        "no chains": dict(num=0),
        "too many chains": dict(chains=(good,) * 9),
        "negative link": dict(chains=(edited(link=-1),)),
        "link == L": dict(chains=(edited(link=c.L),)),
        "num_dofs 0": dict(chains=(edited(num_dofs=0),)),
        "num_dofs 9": dict(chains=(edited(num_dofs=9),)),
        "dof == D": dict(chains=(edited(dofs=[c.D]),)),
        "negative dof": dict(chains=(edited(dofs=[0, -1]),)),
        "dof twice": dict(chains=(edited(dofs=[1, 2, 1]),)),
        "bad second chain": dict(chains=(good, edited(link=c.L))),
        "damping 0": dict(damping=0.0),
        "damping negative": dict(damping=-0.3),
        "damping nan": dict(damping=float("nan")),
        "damping inf": dict(damping=float("inf")),
        "no output": dict(out=None),
    }
    for what, kw in bad.items():
        rc, msg = call(**kw)
        assert rc == -1, (what, rc)                                        # TG_ERR_ARG
        assert msg.startswith(b"tg_ik_dls:"), (what, msg)
    torch.cuda.synchronize()


def test_python_argument_checks():
    c = shared("thormang")
    s = c.s
    with pytest.raises(ValueError):
        s.solve_ik(c.chains, c.gp_t[:, :2], c.gq_t)                        # shape
    with pytest.raises(ValueError):
        s.solve_ik(c.chains, c.gp_t.double(), c.gq_t)                      # dtype
    with pytest.raises(ValueError):
        s.solve_ik(c.chains, c.gp_t.cpu(), c.gq_t)                         # device
    with pytest.raises(ValueError):
        s.solve_ik(c.chains, c.gp_t.transpose(0, 1).contiguous().transpose(0, 1), c.gq_t)   # contiguity
    with pytest.raises(ValueError):
        s.solve_ik(c.chains, c.gp_t, c.gq_t, targets=torch.zeros(N, c.D + 1, device="cuda:0"))
    with pytest.raises(KeyError):
        s.ik_chain("no_such_link")
    with pytest.raises(ValueError):
        s.ik_chain("l_arm_end_link", num_dofs=9)
    ch = s.ik_chain("l_arm_end_link", num_dofs=7)
    assert [c.m.dof_names[ch.dofs[i]] for i in range(7)] == ["l_arm_sh_p1", "l_arm_sh_r", "l_arm_sh_p2", "l_arm_el_y",
                                                             "l_arm_wr_r", "l_arm_wr_y", "l_arm_wr_p"]
    assert C.sizeof(ch) == 52
