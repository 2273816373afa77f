"""Force sensor tensor (tg_set_force_sensor_tensor) on the GPU.

* single rigid bodies (kat_box, kat_sphere; plane and constant slope, both
  solvers, substeps 1 and 2): the force part is the net contact force tensor's
  row bit for bit; the moment obeys the transport identity between two
  sensors on the link and the angular momentum identity I dw = dt n about the
  centre of mass; local space is R_l^T times env space;
* articulated models: the moments against the fp64 oracle's multipliers on a
  float64 rebuild of the row geometry, the whole-body momentum identities from
  the centroidal state, and the structure the solver guarantees;
* nothing else moves: states and the other two tensors are bit-identical in
  every on / off combination, call sequences agree with fresh sims, argument
  errors change nothing.

Batches are ragged against the workgroup (35 envs: three workgroups of 16, the
whole-body model's 8: five) with a different state per env."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import call_sequences as cs
from tests import physics_models as pm
from tests.force_sensor_ref import box_patch_rows, torus_patch_rows, transport, wrench_at
from tests.oracle_lib import lib as oracle_lib, physics_step
from tests.test_gpu_contact_force import (G, N, THETA, _articulated, _body_sim, _body_state, _row_layout, qrot, ulp32)

pytestmark = pytest.mark.gpu

TG_ERR_ARG, TG_ERR_MODEL = -1, -3
#: two sensor points on the body besides its centre of mass (link frame, m)
OFF_A, OFF_B = (0.05, -0.03, 0.02), (-0.08, 0.06, -0.04)
#: the farthest contact point from the centre of mass: the box's half diagonal, the sphere's radius
EXTENT = {"box": float(np.linalg.norm([0.1, 0.075, 0.05])), "sphere": 0.1}
INERTIA = {"box": np.array([2.0 / 3 * (0.075 ** 2 + 0.05 ** 2), 2.0 / 3 * (0.1 ** 2 + 0.05 ** 2),
                            2.0 / 3 * (0.1 ** 2 + 0.075 ** 2)]), "sphere": np.full(3, 0.4 * 1.0 * 0.1 ** 2)}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _off(s):
    """an empty sensor list turns the tensor off"""
    t = s.acquire_force_sensor_tensor([])
    assert t.shape == (s.num_envs, 0, 6) and s.force_sensor is None


# ------------------------------------------------------------------ single rigid bodies
_SINGLE = {}
CASES = {"box": ("rest", "land", "slide", "twist"), "sphere": ("rest", "land", "spin")}


def _single(ground, solver, substeps):
    """Every start case of both bodies run once per (ground, solver, substeps)
    and shared by the tests below: the start state, the state after one
    simulate, the net contact force tensor and the sensor tensor in env and in
    local space (the same start state simulated twice, the sensors
    re-registered in between).  Sensors: the centre of mass, OFF_A, OFF_B.
    ``twist`` (box): resting, spinning about its vertical principal axis."""
    key = (ground, solver, substeps)
    if key in _SINGLE:
        return _SINGLE[key]
    rs = np.random.default_rng(7)
    out = {}
    for shape, d in (("box", 0.05), ("sphere", 0.1)):
        s, mass, dt, mu = _body_sim(shape, ground, solver, substeps)
        cf = s.acquire_net_contact_force_tensor()
        frames = [s.contact_frame(0), s.contact_frame(0, OFF_A), s.contact_frame("b", OFF_B)]
        for case in CASES[shape]:
            root, nrm = _body_state(rs, "rest" if case == "twist" else case, ground, d)
            if case == "twist":
                root[:, 10:13] = (rs.uniform(1.0, 4.0, (N, 1)) * rs.choice([-1.0, 1.0], (N, 1)) * nrm).astype(np.float32)
            r = {"root": root, "nrm": nrm, "mass": mass, "dt": dt, "mu": mu}
            for space in ("env", "local"):
                fs = s.acquire_force_sensor_tensor(frames, space=space)
                assert fs.shape == (N, 3, 6) and fs is s.acquire_force_sensor_tensor(frames, space=space)
                assert float(fs.abs().max()) == 0.0, "zeros until the first simulate"
                s.root_state.copy_(torch.from_numpy(root))
                s.simulate()
                r[space] = _np(fs)
                r["fs32_" + space] = fs.clone()
                r["cf32_" + space] = cf.clone()
                r["after_" + space] = s.root_state.cpu().numpy().copy()
            out[(shape, case)] = r
        # free flight above the contact distance: exactly 0, and the tensor is rewritten
        assert float(fs.abs().max()) > 0
        root = root.copy()
        root[:, 2] += 1.0
        s.root_state.copy_(torch.from_numpy(root))
        s.simulate()
        assert float(fs.abs().max()) == 0.0
        s.close()
    _SINGLE[key] = out
    return out


GROUNDS = ["flat", "slope_mu0", "slope_mu1"]


@pytest.mark.parametrize("substeps", [1, 2])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("ground", GROUNDS)
def test_force_part_is_the_net_contact_force_bit_for_bit(ground, solver, substeps):
    """Both tensors on: out[..., :3] in env space is the net contact force
    tensor's row of the link, the same sums from the same launch -- for every
    sensor on the link, whatever its offset.  The states after the env-space
    and the local-space run are the same bits too (the sensor never feeds back)."""
    _cuda()
    for (shape, case), r in _single(ground, solver, substeps).items():
        fs, cf = r["fs32_env"], r["cf32_env"]
        assert bool(torch.isfinite(fs).all())
        assert float(cf[:, 0, :].abs().max()) > 0, (shape, case)
        for k in range(3):
            assert torch.equal(fs[:, k, :3], cf[:, 0, :]), (shape, case, k)
        assert torch.equal(r["cf32_env"], r["cf32_local"])
        assert np.array_equal(r["after_env"].view(np.uint32), r["after_local"].view(np.uint32))


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("ground", GROUNDS)
def test_transport_between_two_sensors_on_one_link(ground, solver):
    """substeps = 1: n_B - n_A = (p_A - p_B) x f with the points from the
    start state in float64.  Rounding only: bound 1e-5 L |f| + the float32
    spacing of L |f|, L the largest lever arm involved (the farther sensor's
    distance from the centre of mass plus the body's extent)."""
    _cuda()
    for (shape, case), r in _single(ground, solver, 1).items():
        L = max(np.linalg.norm(OFF_A), np.linalg.norm(OFF_B)) + EXTENT[shape]
        worst = 0.0
        for e in range(N):
            R = qrot(r["root"][e, 3:7].astype(np.float64))
            for a, b, pa, pb in ((1, 2, OFF_A, OFF_B), (0, 1, (0, 0, 0), OFF_A), (0, 2, (0, 0, 0), OFF_B)):
                f = r["env"][e, a, :3]
                res = r["env"][e, b, 3:] - r["env"][e, a, 3:] - np.cross(R @ (np.subtract(pa, pb)), f)
                bound = 1e-5 * L * np.linalg.norm(f) + ulp32(L * np.linalg.norm(f))
                worst = max(worst, np.abs(res).max() / bound)
                assert np.abs(res).max() <= bound, (shape, case, e, a, b, np.abs(res).max(), bound)
        print(ground, solver, shape, case, "transport residual, worst / bound %.3f" % worst)


@pytest.mark.parametrize("substeps", [1, 2])
@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("ground", GROUNDS)
def test_angular_momentum_identity_about_the_centre_of_mass(ground, solver, substeps):
    """The sensor at the centre of mass: I (w_after - w_before) = dt n.  The
    sphere (isotropic inertia) on all of the momentum test's start cases,
    landing, sliding on and spinning; the box from zero angular velocity and
    spinning about its vertical principal axis while resting (no gyroscopic
    term either way; n_z is then the torsion row's alone), at substeps = 1.
    Bound, the form of test_single_body_momentum_identity with I / dt in place
    of m / dt and the sums' terms L |f| in place of |F|:
    64 ulp32(max |w|) I_max / dt + 1e-5 L |f|.  A body resting on the slope
    with friction 1 reads zero moment about the point of the slope under its
    centre of mass."""
    _cuda()
    for (shape, case), r in _single(ground, solver, substeps).items():
        if shape == "box" and substeps != 1:
            continue
        I, dt, L, mass = INERTIA[shape], r["dt"], EXTENT[shape], r["mass"]
        wb = r["root"][:, 10:13].astype(np.float64)
        wa = r["after_env"][:, 10:13].astype(np.float64)
        va = r["after_env"][:, 7:10].astype(np.float64)
        worst = 0.0
        for e in range(N):
            R = qrot(r["root"][e, 3:7].astype(np.float64))
            f, n = r["env"][e, 0, :3], r["env"][e, 0, 3:]
            lhs = R @ (I * (R.T @ (wa[e] - wb[e]))) / dt
            wmax = max(np.abs(wa[e]).max(), np.abs(wb[e]).max())
            bound = 64 * ulp32(wmax) * I.max() / dt + 1e-5 * L * np.linalg.norm(f)
            err = np.abs(lhs - n).max()
            worst = max(worst, err / bound)
            assert err <= bound, (shape, case, e, err, bound)
            if case == "twist" and r["mu"] > 0:
                # the friction rows of a patch at rest under a pure spin carry nothing about the normal:
                # what slows the spin is the torsion row, and it does
                assert abs(n @ r["nrm"]) > 0 and np.sign(n @ r["nrm"]) == -np.sign(wb[e] @ r["nrm"])
            if case == "rest" and ground == "slope_mu1" and shape == "box":
                # zero moment about the slope point vertically under the centre of mass: transported from the
                # centre (lever d / cos(theta) e_z), it differs from n by lever x (f + m g), the residual motion
                lever = np.array([0.0, 0.0, 0.05 / np.cos(THETA)])
                n0 = transport(r["env"][e, 0], R @ np.zeros(3), -lever)[3:]
                slack = bound + I.max() * np.abs(wa[e]).max() / dt + lever[2] * mass * np.abs(va[e]).max() / dt
                assert np.abs(n0).max() <= slack, (e, n0, slack)
        print(ground, solver, substeps, shape, case, "angular momentum identity, worst / bound %.3f" % worst)


@pytest.mark.parametrize("solver", [0, 1])
@pytest.mark.parametrize("ground", GROUNDS)
def test_local_space_is_the_rotated_env_space(ground, solver):
    """substeps = 1: local = R_l^T env, R_l from the start state in float64,
    to the rounding of one rotation: 1e-5 |v| + 4 ulp32(|v|) per vector."""
    _cuda()
    for (shape, case), r in _single(ground, solver, 1).items():
        for e in range(N):
            R = qrot(r["root"][e, 3:7].astype(np.float64))
            for k in range(3):
                for sl in (slice(0, 3), slice(3, 6)):
                    v = r["env"][e, k, sl]
                    nv = np.linalg.norm(v)
                    if sl.start == 3:   # the moment's own rounding scale is that of its terms
                        nv = max(nv, (EXTENT[shape] + np.linalg.norm(OFF_B)) * np.linalg.norm(r["env"][e, k, :3]))
                    assert np.abs(r["local"][e, k, sl] - R.T @ v).max() <= 1e-5 * nv + 4 * ulp32(nv), (shape, case, e, k)


def test_zero_substeps_write_zeros_and_disable_stops_writing():
    _cuda()
    s, mass, dt, mu = _body_sim("box", "flat", 1, 2)
    fs = s.acquire_force_sensor_tensor([0, s.contact_frame(0, OFF_A)], space="local")
    s.refresh_force_sensor_tensor()
    root, _ = _body_state(np.random.default_rng(1), "rest", "flat", 0.05)
    s.root_state.copy_(torch.from_numpy(root))
    s.simulate()
    assert float(fs[:, :, 2].min()) > 0
    sp = s.get_sim_params()
    sub = sp.substeps
    sp.substeps = 0
    s.set_sim_params(sp)
    fs.fill_(float("nan"))
    s.simulate()
    assert float(fs.abs().max()) == 0.0
    sp.substeps = sub
    s.set_sim_params(sp)
    _off(s)
    fs.fill_(-1.0)
    s.simulate()
    assert float(fs.max()) == -1.0 and float(fs.min()) == -1.0
    s.close()


# ------------------------------------------------------------------ articulated models
_ARTFS = {}


def _world_frames(m, root, dofrow, props=None):
    """float64 forward kinematics of one env: per link (R, p) in the world;
    with ``props`` [F, D] the locked DOFs sit at the centre of their window,
    where the simulator holds them"""
    from thormang_isaacgym_amd import abi
    q = {n: float(dofrow[i, 0]) for i, n in enumerate(m.dof_names)}
    if props is not None:
        for d in m.locked_dofs:
            q[m.dof_names[d]] = 0.5 * (float(props[abi.TG_PROP_LOWER, d]) + float(props[abi.TG_PROP_UPPER, d]))
    R0, p0 = qrot(root[3:7].astype(np.float64)), root[0:3].astype(np.float64)
    return [(R0 @ R, p0 + R0 @ p) for R, p in m.forward_kinematics(q)]


def _sensor_set(m, s):
    """One sensor per shape-bearing link at the centre of the face / the point
    of its shape nearest the ground in the link frame (a box: the bottom face;
    a wheel: its centre), a second one on the first of them at an offset, and
    one on a link without shapes."""
    frames, links = [], s.contact_link_indices
    for l in links:
        sh = next(x for x in m.shapes if m.link_index(x.link) == l)
        off = np.asarray(sh.pos, np.float64)
        if sh.kind == "box":
            rot = np.asarray(sh.rot, np.float64).reshape(3, 3)
            k = int(np.argmax(np.abs(rot[2])))
            off = off - np.sign(rot[2, k]) * sh.params[k] * rot[:, k]
        frames.append((l, tuple(float(v) for v in off)))
    frames.append((links[0], tuple(float(v) for v in np.asarray(frames[0][1]) + [0.03, -0.02, 0.04])))
    bare = next(l for l in range(m.num_bodies) if l not in links)
    frames.append((bare, (0.1, 0.2, 0.3)))
    return frames


def _art(name):
    """The start states of tests/test_gpu_contact_force.py (shared, never
    modified) with a Sim of our own at them after one simulate with the
    sensors of _sensor_set on, in env and in local space, beside the net
    contact force tensor."""
    if name in _ARTFS:
        return _ARTFS[name]
    from thormang_isaacgym_amd.sim import Sim
    a = dict(_articulated(name))
    o, m = a["o"], a["m"]
    s = Sim(m, o.sp, N, "cuda:0")

    def start():
        s.root_state.copy_(torch.from_numpy(a["root"]))
        s.dof_state.copy_(torch.from_numpy(a["dof"]))
    start()
    s.dof_props.copy_(torch.from_numpy(a["props"]))
    s.dof_pos_target.copy_(torch.from_numpy(a["pt"]))
    s.dof_vel_target.copy_(torch.from_numpy(a["vt"]))
    s.env_dirty.fill_(1)
    frames = _sensor_set(m, s)
    cf = s.acquire_net_contact_force_tensor()
    res = {}
    for space in ("local", "env"):
        fs = s.acquire_force_sensor_tensor([s.contact_frame(l, off) for l, off in frames], space=space)
        start()
        s.simulate()
        res[space] = _np(fs)
        res["cf_" + space] = cf.clone()
        res["fs32_" + space] = fs.clone()
    a.update(sim2=s, frames=frames, fs=fs, fs_env=res["env"], fs_local=res["local"], res=res, start=start)
    _ARTFS[name] = a
    return a


@pytest.mark.parametrize("name", ["thormang", "gogoro", "thormang_wb"])
def test_articulated_structure(name):
    """What the definition guarantees without a measured tolerance: all values
    finite, every env different, a link without shapes reads 0, the force part
    is the contact tensor's row, f_z >= 0, local = R_l^T env to rounding, the
    centre of pressure of a loaded foot inside the sole's outline, and a full
    rewrite: lifted out of contact, the next simulate writes zeros."""
    _cuda()
    a = _art(name)
    m, s, frames, E, Lc = a["m"], a["sim2"], a["frames"], a["fs_env"], a["fs_local"]
    S = len(frames)
    assert E.shape == (N, S, 6) and np.isfinite(E).all() and np.isfinite(Lc).all()
    assert (E[:, S - 1] == 0).all() and (Lc[:, S - 1] == 0).all(), "a link without shapes"
    assert len({tuple(np.round(E[e].ravel(), 4)) for e in range(N)}) == N, "envs all differ"
    cf = a["res"]["cf_env"]
    for k, (l, _) in enumerate(frames[:-1]):
        assert torch.equal(a["res"]["fs32_env"][:, k, :3], cf[:, l, :]), (k, l)
    assert (E[:, :, 2] >= 0).all()
    assert (E[:, :S - 1, 2].sum(axis=1) > 0).all(), "every env touches the ground"
    assert np.abs(E[:, :, 3:]).max() > 0
    M = sum(l.mass for l in m.links)
    mu_g = float(a["o"].sp.ground_friction)
    for e in range(N):
        fk = _world_frames(m, a["root"][e], a["dof"].reshape(N, -1, 2)[e])
        for k, (l, off) in enumerate(frames[:-1]):
            R = fk[l][0]
            f, n = E[e, k, :3], E[e, k, 3:]
            sh = next(x for x in m.shapes if m.link_index(x.link) == l)
            ext = float(np.linalg.norm(sh.params[:3])) + 0.1
            # (with several substeps the local axes turn between them: the single bodies pin local space)
            for v, w, scale in ((f, Lc[e, k, :3], np.linalg.norm(f)), (n, Lc[e, k, 3:], ext * np.linalg.norm(f))):
                if int(a["o"].sp.substeps) == 1:
                    assert np.abs(w - R.T @ v).max() <= 1e-5 * scale + 4 * ulp32(scale), (e, k)
            # the transport to the second sensor on the first link
            if k == 0:
                pa = fk[l][1] + R @ np.asarray(off)
                pb = fk[l][1] + R @ np.asarray(frames[S - 2][1])
                res = E[e, S - 2, 3:] - n - np.cross(pa - pb, f)
                if int(a["o"].sp.substeps) == 1:
                    assert np.abs(res).max() <= 1e-5 * ext * np.linalg.norm(f) + ulp32(ext * np.linalg.norm(f))
            # centre of pressure in sole coordinates: every row of a box patch acts in the sole's plane, where
            # the sensor lies, so n_x = y f_z and n_y = -x f_z sum over the rows with their local d_z as
            # weights -- the normal rows' are positive, and a friction row's is at most sin(tilt) of its
            # multiplier, itself at most mu times the load: slack mu sin(tilt) x the sole's half diagonal
            if sh.kind == "box" and k < S - 2 and "foot" in m.links[l].name and Lc[e, k, 2] > 0.01 * M * G:
                rot = np.asarray(sh.rot, np.float64).reshape(3, 3)
                kk = int(np.argmax(np.abs(rot[2])))
                assert abs(abs(rot[2, kk]) - 1) < 1e-9, "the sole's normal is the link's z"
                cop = np.array([-Lc[e, k, 4], Lc[e, k, 3]]) / Lc[e, k, 2]
                half = np.abs(rot[:2] @ (np.asarray(sh.params[:3]) * (np.arange(3) != kk)))   # outline in link x, y
                tilt = np.arccos(np.clip(R[2, 2], -1, 1))
                mu = 0.5 * (float(sh.friction) + mu_g)
                # (+ 0.01 rad: what a later substep's start can have turned further at these velocities)
                slack = mu * np.sin(tilt + 0.01) * np.linalg.norm(half) + 1e-6
                assert (np.abs(cop) <= half + slack).all(), (e, k, cop, half, slack)
    # lift out of contact with a root write: zeros on the next simulate
    up = s.root_state.clone()
    up[:, 2] += 2.0
    s.set_actor_root_state_indexed(up, s.all_ids)
    a["fs"].fill_(float("nan"))
    s.simulate()
    assert float(a["fs"].abs().max()) == 0.0
    a["start"]()


def test_wholebody_kneel_loads_the_shin_and_hand_sensors():
    """thormang_wb in the kneel pose of the whole-body tests: after the fall
    the sensors on the shins and the hands read force, in local space."""
    _cuda()
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_kneel_cfg
    env = make_gpu_walk(walk_kneel_cfg(N), NumpyDraws(0))
    m = env.model
    assert m.name == "thormang_wb" and len(m.shapes) == 6
    links = env.sim.contact_link_indices
    fs = env.acquire_force_sensor_tensor([env.sim.contact_frame(l) for l in links], space="local")
    assert fs is env.sim.acquire_force_sensor_tensor([env.sim.contact_frame(l) for l in links], space="local")
    acc = torch.zeros(N, len(links), 6, device="cuda:0")
    act = torch.zeros(N, m.num_dof, device="cuda:0")
    for t in range(150):   # (zero actions: down and at rest after ~100 steps, tests/test_walk_wholebody.py)
        env.step(act)
        if t >= 100:
            acc += fs
    F = _np(acc / 50)
    assert np.isfinite(F).all()
    names = [m.links[l].name for l in links]
    shins = [names.index("l_leg_kn_p_link"), names.index("r_leg_kn_p_link")]
    hands = [names.index("l_arm_wr_p_link"), names.index("r_arm_wr_p_link")]
    M = sum(l.mass for l in m.links)
    fn = np.linalg.norm(F[:, :, :3], axis=2)
    print("kneel: mean |f| shins", fn[:, shins].mean(), "hands", fn[:, hands].mean(), "mean |n| shins",
          np.linalg.norm(F[:, shins, 3:], axis=2).mean())
    assert (fn[:, shins].sum(axis=1) > 0.05 * M * G).all()
    assert (fn[:, hands].sum(axis=1) > 0).all()
    assert (np.linalg.norm(F[:, shins, 3:], axis=2).sum(axis=1) > 0).all()


def _oracle_wrenches(a, e, precision):
    """Env e's sensor wrenches [S, 6] (env space, the last sensor's bare link
    left out) from the oracle's dumped stored-velocity multipliers on a float64
    rebuild of the row geometry on flat ground (tests/force_sensor_ref.py): per
    substep the multipliers of that substep of the full step (one
    single-threaded oracle call per substep index, as _oracle_fz reads them)
    and the geometry from the float64 forward kinematics of the state that
    substep starts from, which a one-substep oracle step of length h advances.

    Of the dump only the multipliers are read.  The separations, and with them
    the weights of the friction anchor, are rebuilt as the float64 heights of
    the corners from that forward kinematics instead of taken from the dump
    (whose entries hold the contact-offset rule's target form under TGS, not
    the raw heights): the fp32 control then shares the float64 geometry, so
    every fp32 error of the GPU's geometry counts against the GPU alone."""
    L = oracle_lib(precision)
    L.oracle_dump_set.argtypes = [C.c_int, C.c_int]
    L.oracle_dump_read.argtypes = [C.c_void_p, C.c_int]
    o, m, D, frames = a["o"], a["m"], a["D"], a["frames"][:-1]
    S, h = int(o.sp.substeps), float(o.sp.dt) / int(o.sp.substeps)
    sp1 = type(o.sp).from_buffer_copy(o.sp)
    sp1.substeps, sp1.dt = 1, h
    layout = _row_layout(m)
    pe = np.ascontiguousarray(a["props"][:, e:e + 1, :])
    rk, dk = a["root"][e:e + 1].copy(), a["dof"][e * D:(e + 1) * D].copy()
    out = np.zeros((len(frames), 6))
    for sub in range(S):
        r, d = a["root"][e:e + 1].copy(), a["dof"][e * D:(e + 1) * D].copy()
        L.oracle_dump_set(0, sub)
        try:
            physics_step(o.desc, o.sp, r, d, pe, a["pt"][e:e + 1].copy(), a["vt"][e:e + 1].copy(), threads=1, L=L)
            buf = np.zeros(4096)
            L.oracle_dump_read(buf.ctypes.data, 4096)
        finally:
            L.oracle_dump_set(-1, 0)
        K = int(buf[0])
        assert K == len(layout), (K, len(layout))
        lam = buf[2500:2500 + K]
        fk = _world_frames(m, rk[0], dk, pe[:, 0, :])
        rows, base = {}, 0
        for sh in m.shapes:
            l = m.link_index(sh.link)
            Rl, pl = fk[l]
            Rs, c = Rl @ np.asarray(sh.rot, np.float64).reshape(3, 3), pl + Rl @ np.asarray(sh.pos, np.float64)
            if sh.kind == "box":
                _, dd, xx, tor = box_patch_rows(Rs, c, sh.params[:3], margin=float(o.sp.contact_margin))
            else:
                assert sh.kind == "torus"
                _, dd, xx, tor = torus_patch_rows(Rs, c, sh.params)
            rows.setdefault(l, []).append((lam[base:base + len(dd)], dd, xx, tor))
            base += len(dd)
        assert base == K
        for k, (l, off) in enumerate(frames):
            p = fk[l][1] + fk[l][0] @ np.asarray(off, np.float64)
            for lm, dd, xx, tor in rows[l]:
                out[k] += wrench_at(p, lm, dd, xx, tor, h) / S
        physics_step(o.desc, sp1, rk, dk, pe, a["pt"][e:e + 1].copy(), a["vt"][e:e + 1].copy(), threads=1, L=L)
    return out


@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_moments_match_the_fp64_oracle(name):
    """Per sensor on a foot or wheel link, the moment about the sensor point
    against the fp64 oracle (_oracle_wrenches).  The yardstick is the
    project's usual one: the GPU's largest error over all 35 envs within 4x
    that of the oracle's own fp32 build on the same quantity, plus
    1e-6 M |g| L, L the largest lever arm (the sensor to the farthest point of
    its link's shape).  The force part is held to the same bar without L."""
    _cuda()
    a = _art(name)
    m = a["m"]
    M = sum(l.mass for l in m.links)
    Lmax = 0.0
    for l, off in a["frames"][:-1]:
        sh = next(x for x in m.shapes if m.link_index(x.link) == l)
        ext = float(np.linalg.norm(sh.params[:3])) if sh.kind == "box" else float(sh.params[0] + sh.params[1])
        Lmax = max(Lmax, ext + float(np.linalg.norm(np.asarray(off) - np.asarray(sh.pos))))
    S = len(a["frames"]) - 1
    eg, ec = np.zeros((N, 2)), np.zeros((N, 2))
    for e in range(N):
        w64, w32 = _oracle_wrenches(a, e, "f64"), _oracle_wrenches(a, e, "f32")
        assert w64[:, 2].max() > 0.05 * M * G, "the env carries weight on the ground"
        g = a["fs_env"][e, :S]
        eg[e] = np.abs(g[:, :3] - w64[:, :3]).max(), np.abs(g[:, 3:] - w64[:, 3:]).max()
        ec[e] = np.abs(w32[:, :3] - w64[:, :3]).max(), np.abs(w32[:, 3:] - w64[:, 3:]).max()
    for i, (what, unit) in enumerate((("force", "N"), ("moment", "N m"))):
        print(name, "%s error vs fp64 oracle over all envs: GPU %.4e %s, fp32 oracle (control) %.4e %s, ratio %.2f; "
              "median env GPU %.4e, control %.4e; M|g| %.1f N, L %.3f m"
              % (what, eg[:, i].max(), unit, ec[:, i].max(), unit, eg[:, i].max() / max(ec[:, i].max(), 1e-30),
                 np.median(eg[:, i]), np.median(ec[:, i]), M * G, Lmax))
    assert eg[:, 0].max() <= 4 * ec[:, 0].max() + 1e-6 * M * G, (eg[:, 0].max(), ec[:, 0].max())
    assert eg[:, 1].max() <= 4 * ec[:, 1].max() + 1e-6 * M * G * Lmax, (eg[:, 1].max(), ec[:, 1].max())


# measured on the MI355X ("The force sensor export"): the largest residuals of the two identities
# over the 35 envs, in N s and N m s, at dt / 8 and over the full dt
MOMENTUM_MEASURED = {"linear": 9.06e-5, "angular": 1.105e-4}
MOMENTUM_MEASURED_FULL_DT = {"linear": 7.17e-4, "angular": 7.02e-3}


def test_whole_body_momentum_identities():
    """thormang, free base, a sensor at the centre of each sole: with c, M c'
    and k from Sim.centroidal() before and after one simulate,
        delta(M c') = dt (M g + sum f_k),
        delta(k) = dt sum ((p_k - c) x f_k + n_k)
    up to the discretisation (p_k and c from the state the simulate starts
    from; the step moves both), so the tolerance is measured: 4x the largest
    residual recorded on the MI355X.  The same identity with every sensor
    offset wrong by 1 cm on the reference side must miss that tolerance by
    10x: the test can fail.

    The states are those of _articulated_state held at their own pose
    (position targets = the start positions) and settled for 20 simulates, so
    that the feet bear the weight and no joint runs into its velocity limit:
    the raw start states pull every joint towards the task's default pose at
    up to 10 rad/s, and the velocity clamp is no force -- the CPU oracle
    misses the linear identity by 1.4 .. 6 N s on them for that reason, and
    closes it to 2e-3 N s on the held ones.

    The 10x assertion is made on a simulate at dt / 8.  The settled robots
    still rock on their feet at up to 0.35 rad/s, and the scheme's own error in
    k -- the momentum matrix of the end pose applied to a velocity update made
    at the start pose, O(h^2 |u|^2 I) -- reads 7.0e-3 N m s over a full dt,
    4.3e-4 at dt / 4 and 1.1e-4 at dt / 8 on the MI355X (the factors 16 and 4
    of h^2), while 1 cm of lever under 430 N changes dt sum (p x f) by 7.2e-2,
    1.8e-2 and 9.4e-3: only in h, so the wrong offsets stand out 10x over 4x
    the residual from dt / 8 on (85x the residual there, 10.7x at the full
    dt).  Measured at dt / 8: linear 9.06e-5 N s, angular 1.105e-4 N m s.

    The task's full dt is asserted too, from the same settled state: both
    residuals within 4x the measured 7.17e-4 N s and 7.02e-3 N m s, and the
    wrong offsets (7.5e-2 N m s) at least 2x that tolerance -- 2.7x is all the
    O(h^2) term leaves there."""
    _cuda()
    a = _art("thormang")
    m, s, frames, D = a["m"], a["sim2"], a["frames"], a["D"]
    a["start"]()
    s.acquire_force_sensor_tensor([s.contact_frame(l, off) for l, off in frames], space="env")
    s.dof_pos_target.copy_(torch.from_numpy(np.ascontiguousarray(a["dof"].reshape(N, D, 2)[:, :, 0])))
    for _ in range(20):
        s.simulate()
    root_t, dof_t = s.root_state.clone(), s.dof_state.clone()
    root0, dof0 = root_t.cpu().numpy(), dof_t.cpu().numpy().reshape(N, D, 2)
    fks = [_world_frames(m, root0[e], dof0[e]) for e in range(N)]
    g = np.array([0.0, 0.0, -G])
    sp = s.get_sim_params()
    full = float(sp.dt)

    def measure(div):
        """the residuals of one simulate of length dt / div from the settled state"""
        s.root_state.copy_(root_t)
        s.dof_state.copy_(dof_t)
        sp.dt = full / div
        s.set_sim_params(sp)
        dt = float(sp.dt)
        c0 = _np(s.centroidal().state)
        s.simulate()
        c1 = _np(s.centroidal().state)
        W = _np(a["fs"])
        sp.dt = full
        s.set_sim_params(sp)
        M = c0[:, 9]
        assert (W[:, :2, 2].sum(axis=1) > 0.5 * M * G).all(), "the feet bear the weight"
        lin = M[:, None] * (c1[:, 3:6] - c0[:, 3:6]) - dt * (M[:, None] * g + W[:, :2, :3].sum(axis=1))
        ang, bad = np.zeros((N, 3)), np.zeros((N, 3))
        for e in range(N):
            tq, tb = np.zeros(3), np.zeros(3)
            for k, (l, off) in enumerate(frames[:2]):
                R, p = fks[e][l]
                f, n = W[e, k, :3], W[e, k, 3:]
                tq += np.cross(p + R @ np.asarray(off) - c0[e, 0:3], f) + n
                tb += np.cross(p + R @ (np.asarray(off) + [0.01, 0.0, 0.0]) - c0[e, 0:3], f) + n
            ang[e] = c1[e, 6:9] - c0[e, 6:9] - dt * tq
            bad[e] = c1[e, 6:9] - c0[e, 6:9] - dt * tb
        rl, ra, rb = np.abs(lin).max(), np.abs(ang).max(), np.abs(bad).max(axis=1)
        print("whole-body momentum at dt / %d: linear residual %.4e N s, angular %.4e N m s; with the offsets 1 cm "
              "off: min over envs %.4e, max %.4e N m s" % (div, rl, ra, rb.min(), rb.max()))
        return rl, ra, rb.max()

    try:
        rl1, ra1, rb1 = measure(1)
        rl8, ra8, rb8 = measure(8)
    finally:
        s.dof_pos_target.copy_(torch.from_numpy(a["pt"]))
        a["start"]()
    assert rl8 <= 4 * MOMENTUM_MEASURED["linear"] and ra8 <= 4 * MOMENTUM_MEASURED["angular"]
    assert rb8 >= 10 * 4 * MOMENTUM_MEASURED["angular"]
    assert rl1 <= 4 * MOMENTUM_MEASURED_FULL_DT["linear"] and ra1 <= 4 * MOMENTUM_MEASURED_FULL_DT["angular"]
    assert rb1 >= 2 * 4 * MOMENTUM_MEASURED_FULL_DT["angular"]


# ------------------------------------------------------------------ nothing else moves
@pytest.mark.parametrize("name", ["thormang", "gogoro"])
def test_states_and_the_other_tensors_do_not_depend_on_the_tensor(name):
    """20 simulates in every on / off combination of the three export tensors:
    root and DOF state bit-identical throughout, and each tensor bit-identical
    in every combination that has it."""
    _cuda()
    from thormang_isaacgym_amd.sim import Sim
    a = _art(name)

    def run(cf_on, df_on, fs_on):
        s = Sim(a["m"], a["o"].sp, N, "cuda:0")
        s.root_state.copy_(torch.from_numpy(a["root"]))
        s.dof_state.copy_(torch.from_numpy(a["dof"]))
        s.dof_props.copy_(torch.from_numpy(a["props"]))
        s.dof_pos_target.copy_(torch.from_numpy(a["pt"]))
        s.dof_vel_target.copy_(torch.from_numpy(a["vt"]))
        s.env_dirty.fill_(1)
        t = {"cf": s.acquire_net_contact_force_tensor() if cf_on else None,
             "df": s.acquire_dof_force_tensor() if df_on else None,
             "fs": s.acquire_force_sensor_tensor([s.contact_frame(l, off) for l, off in a["frames"]], "local")
             if fs_on else None}
        for _ in range(20):
            s.simulate()
        out = {k: v.clone() for k, v in t.items() if v is not None}
        out.update(root=s.root_state.clone(), dof=s.dof_state.clone())
        s.close()
        return out

    runs = {(c, d, f): run(c, d, f) for c in (0, 1) for d in (0, 1) for f in (0, 1)}
    base = runs[(0, 0, 0)]
    assert bool(torch.isfinite(base["root"]).all())
    first = {}
    for key, r in runs.items():
        assert torch.equal(r["root"], base["root"]) and torch.equal(r["dof"], base["dof"]), key
        for k in ("cf", "df", "fs"):
            if k in r:
                assert float(r[k].abs().max()) > 0, (key, k)
                assert torch.equal(r[k], first.setdefault(k, r[k])), (key, k)


def test_walk_task_exposes_the_foot_sensors_and_is_otherwise_unchanged():
    """ThormangWalk with env.enableFootForceSensors, 50 teacher-forced steps.
    Against the task with the net contact force tensor on instead, which runs
    the same separate post-physics launch: obs, reward, resets, time-outs and
    progress identical in every bit.  Against the default task, whose step is
    the fused kernel -- separately optimised fast-math code: resets, time-outs
    and progress identical, obs and reward within the 1e-5 per step the
    project records for fused against separate
    (tests/test_gpu_walk.py test_gpu_walk_fused_step_equals_separate_calls).
    extras["feet_force_sensor"] is the task's force_sensors, the sim's tensor;
    standing, each loaded foot's centre of pressure lies inside its sole."""
    _cuda()
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_cfg
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_centre
    envs = []
    for key in (None, "enableContactForces", "enableFootForceSensors"):
        cfg = walk_cfg(N)
        if key:
            cfg["env"][key] = True
        envs.append(make_gpu_walk(cfg, NumpyDraws(5)))
    off, ctl, on = envs
    assert off.force_sensors is None and "feet_force_sensor" not in off.extras and ctl.force_sensors is None
    assert on.force_sensors.shape == (N, 2, 6) and on.force_sensors is on.sim.force_sensor
    feet = walk_feet_indices(on.model)
    assert on.sim._force_sensor_key == ("local", tuple((l, tuple(float(np.float32(v)) for v in
                                                                 walk_sole_centre(on.model, l))) for l in feet))
    on.refresh_force_sensor_tensor()
    rs = np.random.default_rng(9)
    dobs = drew = seen = 0.0
    flat = 0
    M = sum(l.mass for l in on.model.links)
    half = [np.asarray(next(s for s in on.model.shapes if on.model.link_index(s.link) == l).params[:2]) for l in feet]
    for t in range(50):
        for e in (ctl, on):
            for name in ("obs_buf", "rew_buf", "reset_buf", "progress_buf", "actions", "last_actions", "commands"):
                getattr(e, name).copy_(getattr(off, name))
            e.sim.root_state.copy_(off.sim.root_state)
            e.sim.dof_state.copy_(off.sim.dof_state)
            if off.push_enabled:
                e.sim.body_force.copy_(off.sim.body_force)
        act = torch.from_numpy(rs.uniform(-0.5, 0.5, (N, on.model.num_dof)).astype(np.float32)).cuda()
        if t < 5:
            act.zero_()   # standing on flat feet first
            on.sim.refresh_rigid_body_state_tensor()
            rb0 = _np(on.sim.acquire_rigid_body_state_tensor()).reshape(N, -1, 13)
        o0, r0, z0, x0 = off.step(act.clone())
        oc, rc, zc, xc = ctl.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        assert torch.equal(oc["obs"], o1["obs"]) and torch.equal(rc, r1) and torch.equal(zc, z1)
        assert torch.equal(xc["time_outs"], x1["time_outs"]) and torch.equal(ctl.progress_buf, on.progress_buf)
        assert torch.equal(z0, z1) and torch.equal(x0["time_outs"], x1["time_outs"])
        assert torch.equal(off.progress_buf, on.progress_buf)
        dobs = max(dobs, float((o0["obs"] - o1["obs"]).abs().max()))
        drew = max(drew, float((r0 - r1).abs().max()))
        ff = x1["feet_force_sensor"]
        assert ff.shape == (N, 2, 6) and torch.equal(ff, on.force_sensors) and bool(torch.isfinite(ff).all())
        seen = max(seen, float(ff[:, :, 2].max()))
        if t < 5:
            w = _np(ff)
            on.sim.refresh_rigid_body_state_tensor()
            rb = _np(on.sim.acquire_rigid_body_state_tensor()).reshape(N, -1, 13)
            for k in range(2):
                # a flat-standing foot: loaded, and within 0.05 rad of level before and after the step (a
                # landing foot turns through more than its end poses show); the slack of the structure
                # test from the larger of the two tilts + 0.01 rad
                tilt = np.maximum(*(np.arccos(np.clip(1 - 2 * (x[:, feet[k], 3] ** 2 + x[:, feet[k], 4] ** 2), -1, 1))
                                    for x in (rb0, rb)))
                load = (w[:, k, 2] > 0.05 * M * G) & (tilt < 0.05)
                flat += int(load.sum())
                cop = np.stack([-w[load, k, 4], w[load, k, 3]], 1) / w[load, k, 2:3]
                slack = np.sin(tilt[load] + 0.01)[:, None] * np.linalg.norm(half[k]) + 1e-6   # (mu = 1)
                assert (np.abs(cop) <= half[k] + slack).all(), (t, k)
    print("walk with / without the foot sensors: max |d obs| %.3e, max |d reward| %.3e against the fused step"
          % (dobs, drew))
    print("flat-standing loaded feet checked for their centre of pressure:", flat)
    assert seen > 0.2 * M * G and flat > 0, (seen, flat)
    assert dobs <= 1e-5 and drew <= 1e-5, (dobs, drew)


# ------------------------------------------------------------------ call sequences
def _fresh_copy(monkeypatch, sim, regs, n):
    """A freshly created cache-free sim with everything ``sim``'s next
    simulate reads, and the export tensors registered as ``regs`` says."""
    c = cs.create_under(monkeypatch, cs.CONTROL, lambda: cs.walk_sim(n))
    cs.transplant(sim, c)
    if regs.get("cf"):
        c.acquire_net_contact_force_tensor()
    if regs.get("df"):
        c.acquire_dof_force_tensor()
    if regs.get("fs"):
        frames, space = regs["fs"]
        c.acquire_force_sensor_tensor([c.contact_frame(l, off) for l, off in frames], space)
    return c


def test_call_sequences_agree_with_fresh_sims(monkeypatch):
    """Enable, simulate, re-register with other sensors and the other space,
    disable, re-enable, interleaved with the other two tensors: before every
    simulate a fresh cache-free sim takes over the state and the current
    registrations, and after it root, DOF state and every live tensor agree
    bit for bit.  A stale frame set or launch cache cannot survive that."""
    _cuda()
    n = N
    s = cs.walk_sim(n)
    from thormang_isaacgym_amd.sim import load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_centre
    m = load_model("thormang")
    feet = walk_feet_indices(m)
    A = [(l, tuple(walk_sole_centre(m, l))) for l in feet]
    B = [(feet[1], (0.02, 0.0, -0.01)), (0, (0.0, 0.0, 0.0)), (feet[0], (0.0, 0.03, 0.0)), (feet[0], (0.0, 0.0, 0.0))]
    tg = cs.walk_targets(n, 8)
    regs, seen = {}, {}
    step = [0]

    def sim_and_check(what):
        s.set_dof_position_targets(tg[step[0] % len(tg)])
        c = _fresh_copy(monkeypatch, s, regs, n)
        c.set_dof_position_targets(tg[step[0] % len(tg)])
        step[0] += 1
        s.simulate()
        c.simulate()
        assert torch.equal(s.root_state, c.root_state) and torch.equal(s.dof_state, c.dof_state), what
        for k, attr in (("cf", "net_contact_force"), ("df", "dof_force"), ("fs", "force_sensor")):
            if regs.get(k):
                x, y = getattr(s, attr), getattr(c, attr)
                seen[k] = max(seen.get(k, 0.0), float(x.abs().max()))
                assert torch.equal(x, y), (what, k, float((x - y).abs().max()))
        c.close()

    def reg(frames, space):
        regs["fs"] = (frames, space)
        return s.acquire_force_sensor_tensor([s.contact_frame(l, off) for l, off in frames], space)

    sim_and_check("plain")
    t1 = reg(A, "env")
    sim_and_check("A env")
    sim_and_check("A env again")
    regs["cf"] = True
    s.acquire_net_contact_force_tensor()
    sim_and_check("A env + cf")
    t2 = reg(B, "local")
    assert t2 is not t1 and t2.shape == (n, 4, 6)
    keep = t1.clone()
    sim_and_check("B local + cf")
    assert torch.equal(t1, keep), "the earlier tensor is no longer written"
    regs["df"] = True
    s.acquire_dof_force_tensor()
    sim_and_check("B local + cf + df")
    _off(s)
    regs.pop("fs")
    t2.fill_(-1.0)
    sim_and_check("cf + df, sensors off")
    assert float(t2.max()) == -1.0 and float(t2.min()) == -1.0
    cs.contact_tensor_off(s)
    regs.pop("cf")
    t3 = reg(A, "local")
    sim_and_check("A local + df")
    cs.dof_force_tensor_off(s)
    regs.pop("df")
    sim_and_check("A local alone")
    t4 = reg(A, "env")
    assert t4 is not t3
    sim_and_check("A env alone")
    assert all(seen[k] > 0 for k in ("cf", "df", "fs")), seen
    s.close()


def test_fused_task_steps_interleaved_agree_with_the_cache_free_control(monkeypatch):
    """The env-level sequence, after tests/test_gpu_call_sequences.py T3:
    ThormangWalkDR (per-env masses and friction, pushes, timeout resets inside
    the run), 12 steps, run with the default environment and under the
    cache-free control (TG_ALWAYS_COMPOSE=1 TG_NO_SHARED_CACHE=1).  Fused steps
    first; the sensors on before step 2 (sole centres, env space), the contact
    tensor beside them before step 3, re-registered with other sensors in
    local space before step 4, the DOF force tensor on before step 5, the
    sensors off before step 6 (the other two still decline the fused step),
    those off before step 7 -- fused steps again -- the sensors on once more
    before step 9 (local) and off before step 10.  Every step's obs, reward,
    resets, progress, root and DOF state and every live tensor agree bit for
    bit between the two runs, and the launch statistics show which steps ran
    fused.  A composite or launch cache left behind by a fused step, or a stale
    frame set, cannot survive that."""
    _cuda()
    from tests.test_gpu_call_sequences import N as NC, _actions, _make, _pending
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_centre
    acts = _actions(NC, 33, 12, 5, scale=1.2)
    out = []
    for switches in ({}, cs.CONTROL):
        env = _make(monkeypatch, switches, "ThormangWalkDR", NC, 5)
        sim, m = env.sim, env.model
        feet = walk_feet_indices(m)
        A = [sim.contact_frame(l, walk_sole_centre(m, l)) for l in feet]
        B = [sim.contact_frame(feet[1], (0.02, 0.0, -0.01)), sim.contact_frame(0), sim.contact_frame(feet[0], (0.0, 0.03, 0.0))]
        trace, marks, n_reset, tensors = [], [cs.launch_stats(sim)], 0, []
        for t in range(12):
            if t == 2:
                tensors.append(env.acquire_force_sensor_tensor(A, "env"))
            if t == 3:
                sim.acquire_net_contact_force_tensor()
            if t == 4:
                tensors.append(env.acquire_force_sensor_tensor(B, "local"))
                assert tensors[1] is not tensors[0] and tensors[1].shape == (NC, 3, 6)
            if t == 5:
                sim.acquire_dof_force_tensor()
            if t == 6:
                _off(sim)
            if t == 7:
                cs.contact_tensor_off(sim)
                cs.dof_force_tensor_off(sim)
            if t == 9:
                tensors.append(env.acquire_force_sensor_tensor(A, "local"))
            if t == 10:
                _off(sim)
            n_reset += _pending(env)
            env.step(acts[t])
            snap = cs.snap_env(env)
            if sim.force_sensor is not None:
                snap["force_sensor"] = sim.force_sensor.clone()
            trace.append(snap)
            marks.append(cs.launch_stats(sim))
        sim.sync()
        out.append((trace, marks, n_reset, [x.clone() for x in tensors]))
        del env
    (a, ma, ra, ta), (b, mb, rb, tb) = out
    print("fused / sensor sequence: A", ma[-1], "B", mb[-1], "resets", ra)
    assert ra == rb and ra > 0
    cs.assert_same(a, b, "sensor sequence A vs control")
    assert [t for t, s in enumerate(a) if "force_sensor" in s] == [2, 3, 4, 5, 9]
    assert [t for t, s in enumerate(a) if "net_contact_force" in s] == [3, 4, 5, 6]
    assert [t for t, s in enumerate(a) if "dof_force" in s] == [5, 6]
    for t in (2, 3, 4, 5, 9):
        assert float(a[t]["force_sensor"].abs().max()) > 0, t
    # a tensor that was replaced or turned off is no longer written: each keeps its last step's values
    for x, y, last in zip(ta, tb, (3, 5, 9)):
        assert torch.equal(x, y) and torch.equal(x, a[last]["force_sensor"])
    step = [{k: ma[t + 1][k] - ma[t][k] for k in cs.STATS} for t in range(12)]
    for t, d in enumerate(step):
        if 2 <= t < 7 or t == 9:   # declined, then the general path: the pre-physics rides in a full compose
            assert d["declined"] > 0 and d["full"] == 1 and d["skipped"] == 0, (t, d)
        elif t == 0:   # creation
            assert d["declined"] == 0 and d["full"] == 1 and d["skipped"] == 0, (t, d)
        else:          # the fused step, no compose
            assert d["declined"] == 0 and d["full"] == 0 and d["skipped"] == 1, (t, d)
    assert mb[-1]["skipped"] == 0 and mb[-1]["full"] == 12, mb[-1]


# ------------------------------------------------------------------ argument errors
def test_argument_errors_are_rejected_and_change_nothing():
    _cuda()
    from thormang_isaacgym_amd import abi
    from thormang_isaacgym_amd._lib import lib
    s, mass, dt, mu = _body_sim("box", "flat", 1, 1)
    good = [s.contact_frame(0), s.contact_frame(0, OFF_A)]
    fs = s.acquire_force_sensor_tensor(good, space="local")
    root, _ = _body_state(np.random.default_rng(3), "slide", "flat", 0.05)
    s.root_state.copy_(torch.from_numpy(root))
    s.simulate()
    want = fs.clone()
    assert float(want.abs().max()) > 0
    f = lib().tg_set_force_sensor_tensor
    other = torch.full((N, 8, 6), 7.0, device="cuda:0")
    op = C.c_void_p(other.data_ptr())

    def frames(*items):
        return (abi.tg_contact_frame * max(len(items), 1))(*[s.contact_frame(0, o) if not isinstance(o, int) else
                                                              _raw(o) for o in items])

    def _raw(link):
        c = abi.tg_contact_frame()
        c.link = link
        return c
    nanf = frames((0.0, float("nan"), 0.0))
    inff = frames((0.0, 0.0, 0.0), (float("inf"), 0.0, 0.0))
    bad = [("null sim", (None, frames((0, 0, 0)), 1, 0, op)),
           ("num_sensors -1", (s.handle, frames((0, 0, 0)), -1, 0, op)),
           ("num_sensors 9", (s.handle, (abi.tg_contact_frame * 9)(), 9, 0, op)),
           ("null sensors", (s.handle, None, 2, 0, op)),
           ("link -1", (s.handle, frames(-1), 1, 0, op)),
           ("link L", (s.handle, frames(s.L), 1, 0, op)),
           ("nan offset", (s.handle, nanf, 1, 0, op)),
           ("inf offset", (s.handle, inff, 2, 0, op)),
           ("space 2", (s.handle, frames((0, 0, 0)), 1, 2, op)),
           ("space -1", (s.handle, frames((0, 0, 0)), 1, -1, op)),
           ("out with 0 sensors", (s.handle, frames((0, 0, 0)), 0, 0, op))]
    for what, args in bad:
        assert f(*args) == TG_ERR_ARG, what
        assert lib().tg_last_error().startswith(b"tg_set_force_sensor_tensor: "), (what, lib().tg_last_error())
    with pytest.raises(ValueError):
        s.acquire_force_sensor_tensor(good, space="world")
    with pytest.raises(ValueError):
        s.acquire_force_sensor_tensor([s.L])
    # nothing changed: the registration is the one from before, its tensor is rewritten with the same
    # values from the same state, and no rejected call touched its output
    assert s.acquire_force_sensor_tensor(good, space="local") is fs
    fs.fill_(float("nan"))
    s.root_state.copy_(torch.from_numpy(root))
    s.simulate()
    assert torch.equal(fs, want)
    assert float(other.min()) == 7.0 and float(other.max()) == 7.0
    s.close()


def test_jit_model_is_refused_with_a_message():
    _cuda()
    from thormang_isaacgym_amd._lib import lib
    from thormang_isaacgym_amd.sim import Sim
    m = pm.jit_walker()
    desc, sp, *_ = pm.sim(m, n=4)
    s = Sim(m, sp, 4, "cuda:0")
    assert s.jit
    t = torch.full((4, 1, 6), 5.0, device="cuda:0")
    fr = (s.contact_frame(0),)
    from thormang_isaacgym_amd import abi
    rc = lib().tg_set_force_sensor_tensor(s.handle, (abi.tg_contact_frame * 1)(*fr), 1, 0, C.c_void_p(t.data_ptr()))
    assert rc == TG_ERR_MODEL and b"compiled-in" in lib().tg_last_error()
    assert lib().tg_last_error().startswith(b"tg_set_force_sensor_tensor: ")
    with pytest.raises(RuntimeError, match="compiled-in"):
        s.acquire_force_sensor_tensor([0])
    s.simulate()
    assert float(t.min()) == 5.0 and float(t.max()) == 5.0
    s.close()
