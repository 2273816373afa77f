"""Thormang3 flat-ground walking task (registered as "ThormangWalk").

The reference contains no Thormang walking task:
``thormang3.urdf`` is only ridden passively on the scooter and the humanoid
tasks are ``tasks/humanoid.py`` (MJCF) and the stub ``tasks/MA_OP3.py``.  This
task is designed on those patterns -- PD position control with
``control.{stiffness,damping,actionScale}`` and ``defaultJointAngles``
(cfg/task/MA_OP3.yaml:36-60), velocity-command tracking rewards
(MA_OP3.yaml:72-91), DR schema of vec_task.apply_randomizations -- and is
PARITY UNPINNED against the reference.  Its fused kernels (include/tg_walk.h)
are checked against their CPU restatement (oracle/walk_task.c).

Model: thormang3.urdf (44 links, 33 revolute DOFs) with the mesh-derived link
inertias scooter_V13.urdf carries and the xacro's foot boxes
(model/build_models.py); ``env.asset.wholeBodyCollision: true`` adds the
xacro's shin and hand boxes (model ``thormang_wb``).  Actions [N,33] in [-1,1] -> joint targets
default + actionScale * a; observation [N,112] (tg_walk.h).

``env.enableContactForces: true`` (optional, default false) acquires the net
contact force tensor: ``contact_forces`` [N,L,3], ``feet_indices`` and
``extras["feet_contact_force"]`` [N,2,3] after every step, for foot-contact
terms a user adds; observation, reward and reset do not read them.  The step
then runs its post-physics as a separate launch.

``env.enableDofForceSensors: true`` (optional, default false; IsaacGym's
name) acquires the DOF force tensor: ``dof_forces`` [N,D] and
``extras["dof_force"]`` after every step -- the actuators' torques of the last
simulate, for torque, power or saturation terms a user adds.  The reward keeps
its own ``stiffness * (target - q)`` torque term; observation and reset do not
read the tensor either.  The step runs unfused as above.

``env.enableCentroidalState: true`` (optional, default false) adds
``extras["centroidal"]`` [N,16] after every step -- the whole-body centre of
mass, its velocity, the angular momentum about it, the mass and the centroidal
inertia (tgsim.h tg_centroidal) of the state the step returns with, one extra
kernel launch per step -- for CoM height, capture-point or angular-momentum
terms a user adds.  Observation, reward and reset do not read it, and the step
itself is unchanged.

``env.enableFootForceSensors: true`` (optional, default false) registers one
force sensor per foot (tgsim.h tg_set_force_sensor_tensor) at the centre of the
sole -- the centre of the bottom face of the foot's collision box, taken from
the model's shape -- in the foot link's own axes: ``force_sensors`` [N,2,6] and
``extras["feet_force_sensor"]`` after every step, the ground's force on each
foot and its moment about the sole centre, for centre-of-pressure, ZMP or
torsional-load terms a user adds.  Observation, reward and reset do not read
them.  The step runs unfused as above.

``env.enableImu: true`` (optional, default false) adds ``extras["imu"]``
[N,1,20] after every step -- the reading of an inertial measurement unit at
``imu_link`` (tgsim.h tg_imu): the link's quaternion, the projected gravity,
the body-frame velocities, the gyro and accelerometer readings, the angular
acceleration and the valid flag, differenced over ``dt = sim dt x
controlFrequencyInv`` against a history the task keeps, one extra kernel
launch per step.  The masked resets run inside the post-physics kernel
(walk_post_kernel, csrc/walk_task.hip), driven by the ``reset_buf`` the step
before left, which that kernel then overwrites; so the task hands tg_imu a copy
of ``reset_buf`` taken before the step, and an env that was reset during the
step reads ``valid = 0`` and zero accelerations instead of the jump.  An env
reset through ``reset_idx`` from outside has its history dropped, to the same
effect.  Observation, reward and reset do not read the extra, and the step
itself is unchanged.

``env.enableSelfProximity: true`` (optional, default false) adds
``extras["self_proximity"]`` [N,4] after every step -- the summary of tgsim.h
tg_proximity over the default capsule set (``walk_self_capsules``: pelvis,
chest, head and per side upper arm, forearm, hand, thigh, shin and foot) and
the pairs ``Sim.capsule_pairs`` makes of it, of the state the step returns
with: the smallest distance between two limbs, its pair, and the count and
the penalty ``sum max(0, margin - dist)`` under ``env.selfProximityMargin``
(default 0.02 m), one extra kernel launch per step, for a self-collision
penalty or termination a user adds.  At the default stance every pair is clear
of the margin.  Observation, reward and reset do not read the extra, and the
step itself is unchanged.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .. import abi
from .._lib import check, lib
from ..sim import load_model
from .base.vec_task import VecTask


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class ThormangWalk(VecTask):
    #: the walk's template task (MA_OP3) derives from multi_vec_task.MA_VecTask,
    #: whose __parse_sim_params sets contact_offset 0.016 before the cfg keys
    #: (multi_vec_task.py:322)
    default_contact_offset = 0.016
    #: optional DrawSource (uniform(n)/normal(n)) replacing the in-kernel Philox draws
    draw_source = None

    def __init__(self, cfg, rl_device, sim_device, graphics_device_id, headless, virtual_screen_capture, force_render):
        self.cfg = cfg
        self.model = load_model(walk_model_name(cfg))
        D = self.model.num_dof
        cfg["env"]["numObservations"] = abi_num_obs = 13 + 3 * D
        cfg["env"]["numActions"] = D
        self.num_obs_walk = abi_num_obs
        self._rng_counter = 1
        seed = cfg.get("seed", 42)
        self.seed = int(seed) if isinstance(seed, (int, float)) and seed >= 0 else 42
        super().__init__(config=cfg, rl_device=rl_device, sim_device=sim_device,
                         graphics_device_id=graphics_device_id, headless=headless,
                         virtual_screen_capture=virtual_screen_capture, force_render=force_render)
        env = cfg["env"]
        N = self.num_envs
        dev = self.device
        self.dt = float(cfg["sim"]["dt"]) * self.control_freq_inv
        self.max_episode_length = int(math.ceil(env.get("episodeLength_s", 20) / self.dt))
        self.root_tensor = self.sim.root_state
        self.state_dof = self.sim.dof_state
        self.dof_pos = self.state_dof.view(N, D, 2)[..., 0]
        self.dof_vel = self.state_dof.view(N, D, 2)[..., 1]
        self.actions = torch.zeros(N, D, device=dev)
        self.last_actions = torch.zeros(N, D, device=dev)
        self.commands = torch.zeros(N, 3, device=dev)
        self.root_tensor[:, 2] = float(env.get("spawnHeight", 0.79))
        self.root_reset_tensor = self.root_tensor.clone()
        self.params = self._params()
        learn = env.get("learn", {})
        push_s = float(learn.get("pushInterval_s", 0.0))
        self.push_enabled = push_s > 0 and float(learn.get("pushForce", 0.0)) > 0
        self._bufs = self._make_buffers()
        # env.enableContactForces: the per-link ground forces of the last
        # simulate (legged tasks' foot-contact terms, tasks/anymal.py:113-117);
        # observation, reward and reset do not use them
        self.contact_forces = self.dof_forces = None
        self.self_proximity = None   # (set before the first _contact_extras below; env.enableSelfProximity)
        if bool(env.get("enableContactForces", False)):
            self.contact_forces = self.acquire_net_contact_force_tensor()
            self.feet_indices = torch.as_tensor(walk_feet_indices(self.model), dtype=torch.long, device=dev)
            self._contact_extras()
        # env.enableDofForceSensors: the actuators' forces of the last simulate
        # (tasks/MA_OP3.py:91,96,275); observation, reward and reset do not use them
        if bool(env.get("enableDofForceSensors", False)):
            self.dof_forces = self.acquire_dof_force_tensor()
            self._contact_extras()
        # env.enableFootForceSensors: the ground's wrench on each foot at the centre of its sole, foot axes
        # (tasks/humanoid.py:80,167-168,243); observation, reward and reset do not use them
        self.force_sensors = None
        if bool(env.get("enableFootForceSensors", False)):
            self.force_sensors = self.acquire_force_sensor_tensor(
                [self.sim.contact_frame(l, walk_sole_centre(self.model, l)) for l in walk_feet_indices(self.model)],
                space="local")
            self._contact_extras()
        # env.enableCentroidalState: com, com velocity, angular momentum, mass and centroidal inertia of the state a
        # step returns with (tg_centroidal); observation, reward and reset do not use them
        self.centroidal_state = None
        if bool(env.get("enableCentroidalState", False)):
            self.centroidal_state = torch.zeros(N, abi.TG_CENTROIDAL_STATE, device=dev)
        # env.enableImu: orientation, projected gravity, gyro and accelerometer at imu_link of the state a step
        # returns with (tg_imu); observation, reward and reset do not use them
        self.imu_raw = None
        if bool(env.get("enableImu", False)):
            self._imu_sensors = [self.sim.contact_frame("imu_link")]
            self.imu_history = self.sim.imu_history(1)
            self.imu_raw = torch.zeros(N, 1, abi.TG_IMU_WIDTH, device=dev)
            self._imu_reset = torch.zeros(N, dtype=torch.int64, device=dev)
        # env.enableSelfProximity: the smallest distance between the robot's own limbs, its pair, and the count and
        # penalty under env.selfProximityMargin of the state a step returns with (tg_proximity); observation, reward
        # and reset do not use them
        if bool(env.get("enableSelfProximity", False)):
            self.self_capsules = walk_self_capsules(self.model)
            self.self_pairs = self.sim.capsule_pairs(self.self_capsules)
            self.self_margin = float(env.get("selfProximityMargin", WALK_SELF_MARGIN))
            self.self_proximity = torch.zeros(N, 4, device=dev)
            # the set never changes: the argument arrays of tg_proximity are built and checked here, once
            self._prox_args = proximity_args(self.self_capsules, self.self_pairs, self.self_margin)
        self.reset_idx(torch.arange(N, device=dev))

    # ------------------------------------------------------------ creation
    def create_sim(self):
        env = self.cfg["env"]
        ao = walk_asset_options(self.cfg)
        self.sim = self.create_sim_object(self.model, ao, env_spacing=float(env.get("envSpacing", 1.0)))
        m = self.model
        self.num_dof = m.num_dof
        self.dof_names = list(m.dof_names)
        self.dof_name_to_id = m.dof_name_to_id()
        self.num_bodies = m.num_bodies
        props, self.kp, self.default_dof_pos = walk_dof_props(m, self.cfg, self.num_envs)
        self.sim.dof_props.copy_(torch.from_numpy(props))
        self.sim.env_dirty.fill_(1)
        if self.cfg["task"].get("randomize", False):
            self.apply_randomizations(self.cfg["task"]["randomization_params"])

    def _params(self) -> abi.tg_walk_params:
        return walk_params(self.cfg, self.model, self.num_envs, self.sim.G, self.dt, self.max_episode_length,
                           float(self.clip_actions), float(self.clip_obs), self.kp, self.default_dof_pos, self.seed)

    def _make_buffers(self) -> abi.tg_walk_buffers:
        b = abi.tg_walk_buffers()
        pairs = dict(obs_buf=self.obs_buf, rew_buf=self.rew_buf, reset_buf=self.reset_buf,
                     progress_buf=self.progress_buf, timeout_buf=self.timeout_buf, actions=self.actions,
                     last_actions=self.last_actions, commands=self.commands, root_reset=self.root_reset_tensor,
                     root=self.sim.root_state, dof_state=self.sim.dof_state, pos_target=self.sim.dof_pos_target,
                     body_force=self.sim.body_force if self.push_enabled else None, env_dirty=self.sim.env_dirty)
        for k, t in pairs.items():
            setattr(b, k, None if t is None else t.data_ptr())
        self._buf_tensors = pairs
        return b

    def _counter(self):
        self._rng_counter += 1
        return self._rng_counter

    def _dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------ hot path
    def pre_physics_step(self, actions):
        a = actions.to(device=self.device, dtype=torch.float32).contiguous()
        self._imu_mark_resets()
        check(lib().tg_walk_pre_physics(self.sim.handle, C.byref(self.params), C.byref(self._bufs), _p(a)),
              "tg_walk_pre_physics")
        self._keep = a
        if self.push_enabled:
            self.sim.apply_body_forces(self.sim.body_force)

    def _reset_draws(self, ids):
        D = self.num_dof
        out = np.zeros((self.num_envs, 4 + 2 * D), np.float32)
        for i in ids:
            out[i] = self.draw_source.uniform(4 + 2 * D)
        return out

    def _post_draws(self):
        """Replay draws of the coming post_physics_step (None: in-kernel Philox)."""
        if self.draw_source is None:
            return None, None
        ids = self.reset_buf.nonzero(as_tuple=False).squeeze(-1).cpu().numpy()
        rd = self._dev(self._reset_draws(ids))
        pd = self._dev(self.draw_source.uniform(3 * self.num_envs).reshape(self.num_envs, 3))
        return rd, pd

    def post_physics_step(self):
        rd, pd = self._post_draws()
        check(lib().tg_walk_post_physics(self.sim.handle, C.byref(self.params), C.byref(self._bufs), _p(rd), _p(pd),
                                         self._counter()), "tg_walk_post_physics")
        self._keep_post = (rd, pd)
        self._contact_extras()

    def _contact_extras(self):
        """extras["feet_contact_force"] [N, n_feet, 3]: the feet's rows of the
        contact force tensor after this step (env.enableContactForces)."""
        if self.contact_forces is not None:
            self.extras["feet_contact_force"] = self.contact_forces[:, self.feet_indices].to(self.rl_device)
        # extras["dof_force"] [N, D]: the DOF force tensor (env.enableDofForceSensors)
        if self.dof_forces is not None:
            self.extras["dof_force"] = self.dof_forces.to(self.rl_device)
        # extras["feet_force_sensor"] [N, 2, 6]: the feet's force sensors (env.enableFootForceSensors)
        if getattr(self, "force_sensors", None) is not None:
            self.extras["feet_force_sensor"] = self.force_sensors.to(self.rl_device)
        # extras["centroidal"] [N, 16]: the centroidal state (env.enableCentroidalState)
        if getattr(self, "centroidal_state", None) is not None:
            self.extras["centroidal"] = self.centroidal(out=self.centroidal_state).state.to(self.rl_device)
        # extras["imu"] [N, 1, 20]: the IMU reading at imu_link (env.enableImu)
        if getattr(self, "imu_raw", None) is not None:
            self.sim.imu(self._imu_sensors, history=self.imu_history, dt=self.dt, reset=self._imu_reset,
                         out=self.imu_raw)
            self.extras["imu"] = self.imu_raw.to(self.rl_device)
        # extras["self_proximity"] [N, 4]: the summary of the self-collision capsules (env.enableSelfProximity)
        if self.self_proximity is not None:
            arr, n_caps, idx, n_pairs, pp = self._prox_args
            check(lib().tg_proximity(self.sim.handle, arr, n_caps, idx, n_pairs, C.byref(pp), None, None,
                                     _p(self.self_proximity)), "tg_proximity")
            self.extras["self_proximity"] = self.self_proximity.to(self.rl_device)

    def _imu_mark_resets(self):
        """The envs the coming step resets, for its IMU reading (env.enableImu): ``reset_buf`` as it stands before
        the step.  The masked resets run inside the post-physics kernel (walk_post_kernel, csrc/walk_task.hip),
        which reads the ``reset_buf`` the step before left, replaces the state of the flagged envs and then
        writes the new flags -- so after the step ``reset_buf`` no longer says which envs jumped.  Their velocity
        difference over the step is not an acceleration: tg_imu reports them with ``valid = 0``."""
        if getattr(self, "imu_raw", None) is not None:
            self._imu_reset.copy_(self.reset_buf)

    def step(self, actions):
        if self.dr_randomizations.get("actions", None) or self.dr_randomizations.get("observations", None):
            return super().step(actions)
        # pre_physics_step + control_freq_inv x simulate + post_physics_step in
        # one library call (tg_walk_step: the pre-physics work rides in the
        # first simulate's compose launch); reset_buf is unchanged until the
        # post kernel, so the replay draws are taken first
        a = actions.to(device=self.device, dtype=torch.float32).contiguous()
        rd, pd = self._post_draws()
        self._imu_mark_resets()
        check(lib().tg_walk_step(self.sim.handle, C.byref(self.params), C.byref(self._bufs), _p(a),
                                 self.control_freq_inv, _p(rd), _p(pd), self._counter()), "tg_walk_step")
        self.frame_count += self.control_freq_inv
        self._keep, self._keep_post = a, (rd, pd)
        self.extras["time_outs"] = self.timeout_buf
        self._contact_extras()
        self.obs_dict["obs"] = self.obs_buf
        return self._rl_out()

    def reset_idx(self, env_ids):
        env_ids = torch.as_tensor(env_ids, device=self.device)
        n = int(env_ids.numel())
        if n == 0:
            return
        ids32 = env_ids.to(torch.int32).contiguous()
        rd = self._dev(self._reset_draws(np.sort(env_ids.cpu().numpy()))) if self.draw_source is not None else None
        check(lib().tg_walk_reset_idx(self.sim.handle, C.byref(self.params), C.byref(self._bufs), _p(ids32), n,
                                      _p(rd), self._counter()), "tg_walk_reset_idx")
        self._keep_reset = (ids32, rd)
        # an env reset from outside jumps too: its IMU history is dropped, so its next reading has valid = 0
        if getattr(self, "imu_raw", None) is not None:
            self.imu_history[env_ids.long()] = 0.0


def walk_model_name(cfg) -> str:
    """The compiled model the cfg asks for: ``thormang`` (foot boxes), or with
    ``env.asset.wholeBodyCollision`` ``thormang_wb`` (feet, shins and hands
    collide; model/build_models.py)."""
    return "thormang_wb" if cfg["env"].get("asset", {}).get("wholeBodyCollision", False) else "thormang"


def walk_feet_indices(m) -> list:
    """The foot links (l_leg_foot_link, r_leg_foot_link) among the links that
    carry a collision shape, as indices into ``m.links``."""
    from ..sim import contact_link_indices
    return [i for i in contact_link_indices(m) if "foot" in m.links[i].name]


#: (name, link, child or end points, radius) of the walk's default self-collision set (walk_self_capsules): a child
#: link makes the limb capsule from the link's origin to that child's joint; the per-side rows are mirrored for the
#: right side (l_ -> r_, y -> -y).  The radii (0.03 .. 0.09 m) are set so that every default pair keeps the default
#: margin of 0.02 m at the default stance with 5 mm to spare (asserted in tests/test_proximity_reference.py): the
#: closest there are shin and foot, forearm and hand, pelvis and thigh, three joints apart each.  A capsule is a
#: tube inside its link, for the sign of a distance and its trend, not the link's outline
WALK_SELF_CAPSULES = (
    ("pelvis", "pelvis_link", ((0.0, -0.04, 0.02), (0.0, 0.04, 0.02)), 0.055),
    ("chest", "chest_link", ((0.0, 0.0, 0.04), (0.0, 0.0, 0.2)), 0.09),
    ("head", "head_p_link", ((0.0, 0.045, 0.06), None), 0.08),
)
WALK_SELF_CAPSULES_SIDE = (
    ("upper_arm", "l_arm_sh_p2_link", "l_arm_el_y_link", 0.05),
    ("forearm", "l_arm_el_y_link", "l_arm_wr_r_link", 0.04),
    ("hand", "l_arm_wr_p_link", "l_arm_end_link", 0.03),
    ("thigh", "l_leg_hip_p_link", "l_leg_kn_p_link", 0.06),
    ("shin", "l_leg_kn_p_link", "l_leg_an_p_link", 0.05),
    ("foot", "l_leg_foot_link", ((-0.07, 0.014, -0.02), (0.07, 0.014, -0.02)), 0.03),
)
WALK_SELF_MARGIN = 0.02


def walk_self_capsules(m) -> list:
    """The walk's default self-collision capsules on model ``m`` (thormang, thormang_wb), as ``tg_capsule``: pelvis,
    chest and head, then per side upper arm, forearm, hand, thigh, shin and a foot capsule along the sole."""
    from ..sim import limb_capsule, link_tree, make_capsule
    parent, origin = link_tree(m)
    rows = list(WALK_SELF_CAPSULES)
    for side, sy in (("l_", 1.0), ("r_", -1.0)):
        for name, link, geom, radius in WALK_SELF_CAPSULES_SIDE:
            if not isinstance(geom, str):
                geom = tuple(None if p is None else (p[0], sy * p[1], p[2]) for p in geom)
            else:
                geom = side + geom[2:]
            rows.append((side + name, side + link[2:], geom, radius))
    out = []
    for _name, link, geom, radius in rows:
        l = m.link_index(link)
        out.append(limb_capsule(parent, origin, l, m.link_index(geom), radius) if isinstance(geom, str)
                   else make_capsule(l, geom[0], geom[1], radius))
    return out


def proximity_args(capsules, pairs, margin: float):
    """(capsule array, C, flat pair array, P, params) of a tg_proximity call, for a set that is used every step."""
    if not 1 <= len(capsules) <= abi.TG_PROX_MAX_CAPSULES or not 1 <= len(pairs) <= abi.TG_PROX_MAX_PAIRS:
        raise ValueError(f"{len(capsules)} capsules, {len(pairs)} pairs: tg_proximity takes 1..32 and 1..256")
    arr = (abi.tg_capsule * len(capsules))(*capsules)
    idx = (C.c_int32 * (2 * len(pairs)))(*[int(v) for ab in pairs for v in ab])
    pp = abi.tg_proximity_params()
    pp.margin = float(margin)
    return arr, len(capsules), idx, len(pairs), pp


def walk_sole_centre(m, link: int):
    """The centre of the sole of foot ``link`` in the link's frame: the centre
    of the bottom face (the one facing the link's -z) of its collision box."""
    s = next(s for s in m.shapes if m.link_index(s.link) == link and s.kind == "box")
    rot = np.asarray(s.rot, np.float64).reshape(3, 3)
    k = int(np.argmax(np.abs(rot[2])))          # the box axis along the link's z
    down = -np.sign(rot[2, k]) * rot[:, k]      # its direction towards -z
    return [float(v) for v in np.asarray(s.pos, np.float64) + float(s.params[k]) * down]


def walk_sole_patch(m, link: int):
    """The sole of foot ``link`` as a contact patch of ``Sim.contact_qp``:
    ``(offset, (hx, hy))``, the sole's centre (``walk_sole_centre``) and the half
    extents of its collision box along the link's x and y axes (the box's axes
    are the link's up to a permutation)."""
    s = next(s for s in m.shapes if m.link_index(s.link) == link and s.kind == "box")
    rot = np.asarray(s.rot, np.float64).reshape(3, 3)
    ix, iy = int(np.argmax(np.abs(rot[0]))), int(np.argmax(np.abs(rot[1])))
    return walk_sole_centre(m, link), (float(s.params[ix]), float(s.params[iy]))


def walk_asset_options(cfg) -> dict:
    ao = dict(cfg["env"].get("asset", {}))
    ao.setdefault("ground_friction", 1.0)
    return ao


def walk_dof_props(m, cfg, num_envs):
    """[TG_NUM_PROPS,N,D] PD position drives on every joint (control.stiffness/damping,
    arm/head/torso joints with armStiffness/armDamping), asset armature; plus the
    per-joint stiffness and the default joint angles."""
    env = cfg["env"]
    ctl = env.get("control", {})
    D = m.num_dof
    props = abi.default_dof_props(m, num_envs)
    kp = np.full(D, float(ctl.get("stiffness", 300.0)), np.float32)
    kd = np.full(D, float(ctl.get("damping", 10.0)), np.float32)
    for i, n in enumerate(m.dof_names):
        if "arm" in n or "head" in n or "torso" in n:
            kp[i] = float(ctl.get("armStiffness", kp[i]))
            kd[i] = float(ctl.get("armDamping", kd[i]))
    props[abi.TG_PROP_DRIVE_MODE] = 1
    props[abi.TG_PROP_STIFFNESS] = kp
    props[abi.TG_PROP_DAMPING] = kd
    props[abi.TG_PROP_ARMATURE] = float(walk_asset_options(cfg).get("armature", 0.01))
    default = np.zeros(D, np.float32)
    dni = m.dof_name_to_id()
    for n, v in env.get("defaultJointAngles", {}).items():
        default[dni[n]] = v
    return props, kp, default


def walk_params(cfg, m, num_envs, num_groups, dt, max_episode_length, clip_actions, clip_obs, kp, default,
                seed) -> abi.tg_walk_params:
    env = cfg["env"]
    learn = env.get("learn", {})
    rng = env.get("randomCommandVelocityRanges", {})
    D = m.num_dof
    p = abi.tg_walk_params()
    p.num_envs, p.num_dof, p.num_obs, p.num_groups = num_envs, D, 13 + 3 * D, num_groups
    p.action_scale = float(env.get("control", {}).get("actionScale", 0.5))
    p.clip_actions = clip_actions
    p.clip_obs = clip_obs
    p.lin_vel_scale = float(learn.get("linearVelocityScale", 2.0))
    p.ang_vel_scale = float(learn.get("angularVelocityScale", 0.25))
    p.dof_pos_scale = float(learn.get("dofPositionScale", 1.0))
    p.dof_vel_scale = float(learn.get("dofVelocityScale", 0.05))
    p.cmd_vx[:] = rng.get("linear_x", [0.0, 0.6])
    p.cmd_vy[:] = rng.get("linear_y", [-0.2, 0.2])
    p.cmd_wz[:] = rng.get("yaw", [-0.5, 0.5])
    p.rew_lin_vel_xy = float(learn.get("linearVelocityXYRewardScale", 1.0))
    p.rew_ang_vel_z = float(learn.get("angularVelocityZRewardScale", 0.5))
    p.rew_upright = float(learn.get("uprightRewardScale", 0.2))
    p.rew_alive = float(learn.get("aliveReward", 0.5))
    p.rew_height = float(learn.get("heightRewardScale", 0.3))
    p.rew_action_rate = float(learn.get("actionRateRewardScale", -0.01))
    p.rew_dof_vel = float(learn.get("dofVelocityRewardScale", -1e-4))
    p.rew_torque = float(learn.get("torqueRewardScale", -2.5e-6))
    p.rew_termination = float(learn.get("terminationReward", -10.0))
    p.target_height = float(learn.get("targetHeight", 0.78))
    p.termination_height = float(learn.get("terminationHeight", 0.5))
    p.termination_up = float(learn.get("terminationUp", 0.5))
    p.spawn_height = float(env.get("spawnHeight", 0.79))
    p.joint_noise = float(env.get("jointNoise", 0.05))
    push_s = float(learn.get("pushInterval_s", 0.0))
    p.push_force = float(learn.get("pushForce", 0.0)) if push_s > 0 else 0.0
    p.push_interval = max(1, int(round(push_s / dt))) if push_s > 0 else 0
    p.max_episode_length = int(max_episode_length)
    p.dt = float(dt)
    p.default_pos[:D] = [float(x) for x in default]
    p.stiffness[:D] = [float(x) for x in kp]
    p.seed = int(seed)
    return p
