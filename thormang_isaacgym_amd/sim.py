"""Python face of one libtgsim simulation: the part of ``gymapi.Gym`` the
reference tasks use (create_sim/load_asset/create_actor, the tensor API,
simulate), with torch tensors as zero-copy state views.

Reference calls mirrored (isaacgymenvs/tasks/...):
  acquire_actor_root_state_tensor / acquire_dof_state_tensor + wrap_tensor
      -> Sim.root_state [N,13], Sim.dof_state [N*D,2]      (gogoro_new.py:125-130)
  refresh_*_tensor -> Sim.refresh() (state is live: nothing copied; REQUIRED after writes
      through the dof_props / env_dirty views, which take effect at the next simulate only
      after it -- the library skips the compose launch while no env can be dirty)  (gogoro_new.py:141-142)
  set_dof_position/velocity_target_tensor -> Sim.set_dof_*_targets (gogoro_new.py:364,369)
  set_actor_root_state_tensor_indexed / set_dof_state_tensor_indexed  (gogoro_new.py:547,552)
  set_actor_dof_properties (per env)   -> Sim.set_dof_properties_indexed (gogoro_new.py:294,601)
  simulate / fetch_results             -> Sim.simulate / Sim.sync (vec_task.py:335,339)
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import abi
from ._lib import check, lib
from .model.urdf import Model

HERE = os.path.dirname(os.path.abspath(__file__))
COMPILED = os.path.join(HERE, "model", "compiled")


def load_model(name: str) -> Model:
    with open(os.path.join(COMPILED, f"{name}.json")) as f:
        return Model.from_json(f.read())


def load_asset(path: str, name: str | None = None, locked=(), extra_shapes=(), mesh_root: str | None = None,
               shape_friction: dict | None = None) -> Model:
    """gym.load_asset of a URDF at run time (the reference: tasks/gogoro_new.py:198-213):
    parse the file, merge fixed and ``locked`` joints into rigid groups.  A
    ``Sim`` over a model that is not compiled into libtgsim.so compiles its
    kernels on first use (``ensure_specialisation``), so any URDF runs without
    a library rebuild."""
    from .model.urdf import load_urdf
    m = load_urdf(path, name or os.path.splitext(os.path.basename(path))[0], mesh_root=mesh_root,
                  extra_shapes=list(extra_shapes), shape_friction=shape_friction)
    m.build_groups(list(locked))
    return m


def jit_cache_dir() -> str:
    """Where run-time specialisations are cached (TG_JIT_CACHE, default
    ~/.cache/thormang_isaacgym_amd/jit)."""
    d = os.environ.get("TG_JIT_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "thormang_isaacgym_amd",
                                                        "jit")
    os.makedirs(d, exist_ok=True)
    return d


def compiled_model_hashes() -> set:
    n = int(lib().tg_compiled_model_hashes(None, 0))
    arr = (C.c_uint64 * max(n, 1))()
    lib().tg_compiled_model_hashes(arr, n)
    return {int(arr[i]) for i in range(n)}


def ensure_specialisation(model: Model, desc: abi.ModelDesc | None = None) -> bool:
    """Make sure libtgsim can step ``model``: a no-op for a compiled-in model;
    otherwise the model's constexpr tables (model/codegen.py) are compiled by
    hipRTC for gfx950 inside the library (tg_model_jit, cached on disk by hash)
    and registered.  Returns True when a run-time specialisation is used."""
    from .model import codegen
    desc = desc or abi.ModelDesc(model)
    if desc.hash in compiled_model_hashes():
        return False
    cname = "Model_jit_%016x" % desc.hash
    src = codegen.emit(model, cname)
    check(lib().tg_model_jit(C.c_uint64(desc.hash), cname.encode(), src.encode(), None, jit_cache_dir().encode()),
          "tg_model_jit (run-time load_asset)")
    return True


class NativeModel:
    """gym.load_asset through the C ABI alone (tg_model_load, csrc/model_load.cpp):
    the library parses the URDF, builds the tg_model_desc and the
    specialisation's traits and (``jit=True``) compiles them with hipRTC -- what
    a caller without Python gets; ``Sim`` accepts it in place of a ``Model``.
    The descriptor arrays live in the library until the object is freed."""

    def __init__(self, path: str, locked=(), mesh_root: str | None = None, name: str | None = None,
                 jit: bool = True):
        L = lib()
        h = C.c_void_p()
        names = (C.c_char_p * max(len(locked), 1))(*[n.encode() for n in locked])
        args = [path.encode(), name.encode() if name else None, names, len(locked),
                mesh_root.encode() if mesh_root else None]
        rc = L.tg_model_load(*args, jit_cache_dir().encode(), C.byref(h)) if jit else \
            L.tg_model_parse(*args, C.byref(h))
        if rc != 0:
            raise RuntimeError(f"tg_model_load({path}): {L.tg_model_last_error().decode()} (rc {rc})")
        self._h = h
        self.desc = abi.tg_model_desc()
        check(L.tg_model_get_desc(h, C.byref(self.desc)), "tg_model_get_desc")
        self.hash = int(self.desc.model_hash)
        self.num_bodies, self.num_dof = self.desc.num_links, self.desc.num_dofs
        self.num_groups, self.num_shapes = self.desc.num_groups, self.desc.num_shapes
        self.dof_names = [L.tg_model_dof_name(h, i).decode() for i in range(self.num_dof)]
        self.link_names = [L.tg_model_link_name(h, i).decode() for i in range(self.num_bodies)]
        S = self.num_shapes
        self.arrays = {"shape_friction": np.ctypeslib.as_array(self.desc.shape_friction, (S,)).astype(np.float32)
                       if S else np.zeros(0, np.float32)}
        self.jit = jit and self.hash not in compiled_model_hashes()

    def source(self) -> str:
        return lib().tg_model_source(self._h).decode()

    def __del__(self):
        if getattr(self, "_h", None):
            lib().tg_model_free(self._h)
            self._h = None


def contact_link_indices(model) -> list:
    """The links of ``model`` (a ``Model`` or ``NativeModel``) that carry a
    collision shape, ascending, as indices into ``model.links`` order: the
    rows of the net contact force tensor that can be nonzero."""
    if isinstance(model, NativeModel):
        links = [int(model.desc.shape_link[i]) for i in range(model.num_shapes)]
    else:
        links = [model.link_index(s.link) for s in model.shapes]
    return sorted(set(links))


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


Centroidal = namedtuple("Centroidal", ["state", "matrix", "bias"])   # what Sim.centroidal returns
ContactDynamics = namedtuple("ContactDynamics", ["tau", "wrench"])   # what Sim.contact_inverse_dynamics returns
ContactForces = namedtuple("ContactForces", ["tau", "wrench", "forces", "info"])   # what Sim.contact_qp returns
HeightScan = namedtuple("HeightScan", ["heights", "normals"])   # what Sim.height_scan returns
RayCast = namedtuple("RayCast", ["dist", "normals"])   # what Sim.ray_cast returns
Proximity = namedtuple("Proximity", ["dist", "witness", "summary"])   # what Sim.proximity returns


def link_tree(model):
    """(parent [L], joint origin position in the parent frame [L, 3]) of a model, read from its tg_model_desc: what
    ``limb_capsule`` and ``capsule_pairs`` take.  ``model``: a ``Model``, or what owns a descriptor already (a
    ``NativeModel``, an ``abi.ModelDesc``, a ``Sim``'s ``desc``)."""
    owner = model if hasattr(model, "desc") else abi.ModelDesc(model)   # (kept alive while its arrays are read)
    d = owner.desc
    L = int(d.num_links)
    parent = [int(d.link_parent[l]) for l in range(L)]
    origin = np.array([[float(d.link_origin[12 * l + 9 + k]) for k in range(3)] for l in range(L)],
                      np.float64).reshape(L, 3)
    return parent, origin


def make_capsule(link: int, p0, p1=None, radius: float = 0.05) -> abi.tg_capsule:
    """The tg_capsule on link index ``link`` (``p1=None``: a sphere about ``p0``)."""
    p0 = [float(v) for v in p0]
    p1 = p0 if p1 is None else [float(v) for v in p1]
    radius = float(radius)
    if len(p0) != 3 or len(p1) != 3 or not all(math.isfinite(v) for v in p0 + p1):
        raise ValueError("a capsule's end points are three finite numbers each")
    if not (math.isfinite(radius) and radius >= 0.0):
        raise ValueError(f"a capsule's radius is a finite number >= 0, got {radius}")
    c = abi.tg_capsule()
    c.link = int(link)
    c.p0[:], c.p1[:], c.radius = p0, p1, radius
    return c


def limb_capsule(parent, origin, link: int, child: int, radius: float) -> abi.tg_capsule:
    """The capsule from link ``link``'s origin to the origin of the joint that carries ``child`` (``link_tree``)."""
    if parent[child] != link:
        raise ValueError(f"link {child} is carried by link {parent[child]}, not by link {link}")
    return make_capsule(link, (0.0, 0.0, 0.0), origin[child], radius)


def link_hops(parent, a: int, b: int) -> int:
    """The number of joints on the path between links ``a`` and ``b`` of the tree."""
    up = {}
    k, n = a, 0
    while k >= 0:
        up[k] = n
        k, n = parent[k], n + 1
    k, n = b, 0
    while k not in up:
        k, n = parent[k], n + 1
    return up[k] + n


def capsule_pairs(parent, capsules, min_hops: int = 3) -> list:
    """The pairs (a, b), a < b, of ``capsules`` whose links are at least ``min_hops`` joints apart (``link_tree``)."""
    pairs = [(a, b) for a in range(len(capsules)) for b in range(a + 1, len(capsules))
             if link_hops(parent, int(capsules[a].link), int(capsules[b].link)) >= int(min_hops)]
    if len(pairs) > abi.TG_PROX_MAX_PAIRS:
        raise ValueError(f"{len(pairs)} pairs: a proximity call takes at most {abi.TG_PROX_MAX_PAIRS}")
    return pairs
# what Sim.imu returns: views of raw [N, S, 20]
Imu = namedtuple("Imu", ["quat", "gravity", "lin_vel", "ang_vel", "lin_acc", "ang_acc", "valid", "raw"])


class Sim:
    def __init__(self, model: Model, params: abi.tg_sim_params, num_envs: int, device: str = "cuda:0",
                 jit_hash: int | None = None):
        """``jit_hash`` (test hook): register the model under this hash instead
        of its own, so even a compiled-in model runs on a run-time
        (tg_model_jit) specialisation -- the JIT path can then be compared
        with the compiled one on identical inputs."""
        if not device.startswith("cuda"):
            raise RuntimeError(f"libtgsim runs on an MI355X ('cuda:N' device), got {device!r}; "
                               "there is no CPU physics path outside the test oracle")
        self.device = torch.device(device)
        self.model = model
        self.num_envs = N = int(num_envs)
        self.params = params
        torch.cuda.set_device(self.device)
        if isinstance(model, NativeModel):   # loaded (and compiled) by the library itself
            self.desc = model
            self.D, self.G, self.L, self.S = model.num_dof, model.num_groups, model.num_bodies, model.num_shapes
            self.jit = model.jit
        else:
            self.desc = abi.ModelDesc(model)
            if jit_hash is not None:
                self.desc.hash = int(jit_hash)
                self.desc.desc.model_hash = int(jit_hash)
            self.D, self.G, self.L, self.S = model.num_dof, model.num_groups, model.num_bodies, len(model.shapes)
            self.jit = ensure_specialisation(model, self.desc)
        h = C.c_void_p()
        check(lib().tg_sim_create(C.byref(self.desc.desc), C.byref(params), N, self.device.index or 0, C.byref(h)),
              "tg_sim_create")
        self._h = h
        # the force sensor tensor and what it was registered with (acquire_force_sensor_tensor); None: off
        self.force_sensor = None
        self._force_sensor_key = None
        self.stream = torch.cuda.current_stream(self.device)
        check(lib().tg_set_stream(self._h, C.c_void_p(self.stream.cuda_stream)), "tg_set_stream")
        f32 = dict(dtype=torch.float32, device=self.device)
        D, G = self.D, self.G
        self.root_state = torch.zeros(N, 13, **f32)
        self.dof_state = torch.zeros(N * D, 2, **f32)
        self.dof_pos_target = torch.zeros(N, D, **f32)
        self.dof_vel_target = torch.zeros(N, D, **f32)
        self.dof_actuation = torch.zeros(N, D, **f32)
        self.dof_props = torch.zeros(abi.TG_NUM_PROPS, N, D, **f32)
        self.body_force = torch.zeros(N, G, 6, **f32)
        self.env_origin = torch.zeros(N, 3, **f32)
        self.env_dirty = torch.zeros(N, dtype=torch.uint8, device=self.device)
        v = abi.tg_state_view()
        for k in ("root_state", "dof_state", "dof_pos_target", "dof_vel_target", "dof_actuation", "dof_props",
                  "body_force", "env_origin", "env_dirty"):
            setattr(v, k, getattr(self, k).data_ptr())
        check(lib().tg_bind_state(self._h, C.byref(v)), "tg_bind_state")
        self.all_ids = torch.arange(N, dtype=torch.int32, device=self.device)
        # mirrors of the per-env properties the library holds (read back by
        # get_* style inspection and the parity harness; never on the hot path)
        self.body_mass_scale = torch.ones(N, self.L, **f32)
        self.shape_friction = torch.as_tensor(np.asarray(self.desc.arrays["shape_friction"], np.float32),
                                              device=self.device).repeat(N, 1)
        self.gravity = [float(x) for x in params.gravity]

    @property
    def handle(self):
        return self._h

    # ---------------------------------------------------------------- tensor API
    def refresh(self):
        """refresh_*_tensor: the views are live, nothing is copied.  Call it after
        writing through ``dof_props`` / ``env_dirty`` (tg_refresh re-arms the
        compose launch those writes need)."""
        check(lib().tg_refresh(self._h), "refresh")

    def set_dof_position_targets(self, t: torch.Tensor):
        check(lib().tg_set_dof_position_targets(self._h, _ptr(self._dev(t))), "set_dof_position_target_tensor")

    def set_dof_velocity_targets(self, t: torch.Tensor):
        check(lib().tg_set_dof_velocity_targets(self._h, _ptr(self._dev(t))), "set_dof_velocity_target_tensor")

    def set_dof_actuation_forces(self, t: torch.Tensor):
        check(lib().tg_set_dof_actuation_forces(self._h, _ptr(self._dev(t))), "set_dof_actuation_force_tensor")

    def set_actor_root_state_indexed(self, root: torch.Tensor, ids: torch.Tensor):
        ids = self._ids(ids)
        check(lib().tg_set_actor_root_state_indexed(self._h, _ptr(self._dev(root)), _ptr(ids), ids.numel()),
              "set_actor_root_state_tensor_indexed")
        return True

    def set_dof_state_indexed(self, dof: torch.Tensor, ids: torch.Tensor):
        ids = self._ids(ids)
        check(lib().tg_set_dof_state_indexed(self._h, _ptr(self._dev(dof)), _ptr(ids), ids.numel()),
              "set_dof_state_tensor_indexed")
        return True

    def set_dof_properties_indexed(self, field: int, vals: torch.Tensor, ids: torch.Tensor):
        ids = self._ids(ids)
        check(lib().tg_set_dof_properties_indexed(self._h, int(field), _ptr(self._dev(vals)), _ptr(ids),
                                                  ids.numel()), "set_actor_dof_properties")

    def set_body_mass_scale_indexed(self, scale: torch.Tensor, ids: torch.Tensor):
        ids = self._ids(ids)
        check(lib().tg_set_body_mass_scale_indexed(self._h, _ptr(self._dev(scale)), _ptr(ids), ids.numel()),
              "mass scale")
        # host-side mirror of the rigid-body mass properties (get_actor_rigid_body_properties)
        self.body_mass_scale[ids.long()] = scale[ids.long()]

    def set_shape_friction_indexed(self, mu: torch.Tensor, ids: torch.Tensor):
        ids = self._ids(ids)
        check(lib().tg_set_shape_friction_indexed(self._h, _ptr(self._dev(mu)), _ptr(ids), ids.numel()), "friction")
        self.shape_friction[ids.long()] = mu[ids.long()]   # mirror (get_actor_rigid_shape_properties)

    def set_gravity(self, g):
        arr = (C.c_float * 3)(*[float(x) for x in g])
        check(lib().tg_set_gravity(self._h, arr), "set_gravity")
        self.gravity = [float(x) for x in g]

    def apply_body_forces(self, wrench: torch.Tensor):
        """Group wrenches [N, G, 6] (world force, torque about the group com) for the next simulate."""
        check(lib().tg_apply_body_forces(self._h, _ptr(self._dev(wrench))), "apply_body_forces")

    ENV_SPACE, LOCAL_SPACE = 0, 1

    def apply_rigid_body_force_tensors(self, forces, torques=None, space: int = 0):
        """gym.apply_rigid_body_force_tensors(sim, forceTensor, torqueTensor, space)
        (tasks/gogoro_realistic_turning_sim_paper.py:457): forces / torques
        [N*L, 3] (or [N, L, 3]) at the rigid bodies' coms, world (ENV_SPACE) or
        body frame (LOCAL_SPACE), for the next simulate.  Returns True, as gym does."""
        def flat(t):
            if t is None:
                return None
            t = self._dev(t)
            if t.numel() != self.num_envs * self.L * 3:
                raise ValueError(f"rigid-body force tensor must hold N*L*3 = {self.num_envs * self.L * 3} floats, "
                                 f"got shape {tuple(t.shape)}")
            return t.reshape(-1, 3).contiguous()
        f, t = flat(forces), flat(torques)
        check(lib().tg_apply_rigid_body_force_tensors(self._h, _ptr(f), _ptr(t), int(space)),
              "apply_rigid_body_force_tensors")
        self._keep_forces = (f, t)   # the reduction runs on the sim stream; hold the inputs until the next call
        return True

    def set_heightfield(self, heights, horizontal_scale: float = 1.0, vertical_scale: float = 1.0,
                        origin_x: float = 0.0, origin_y: float = 0.0, friction: float = 1.0):
        """gym.add_triangle_mesh of a heightfield trimesh (see tg_set_heightfield); None = flat plane."""
        if heights is None:
            check(lib().tg_set_heightfield(self._h, None, 0, 0, 1.0, 1.0, 0.0, 0.0, 1.0), "set_heightfield")
            return
        if isinstance(heights, torch.Tensor):
            heights = heights.detach().cpu().numpy()
        h = np.ascontiguousarray(np.asarray(heights, np.float32))
        if h.ndim != 2:
            raise ValueError(f"heightfield must be [rows, cols], got shape {h.shape}")
        check(lib().tg_set_heightfield(self._h, h.ctypes.data_as(C.c_void_p), h.shape[0], h.shape[1],
                                       float(horizontal_scale), float(vertical_scale), float(origin_x),
                                       float(origin_y), float(friction)), "set_heightfield")

    def simulate(self):
        check(lib().tg_simulate(self._h), "simulate")

    def debug_fill_lds(self, pattern: int = 0x7FC00000):
        """tg_debug_fill_lds: every CU's LDS filled with ``pattern`` (default a
        quiet NaN) on this sim's stream -- the stale-LDS tests' probe."""
        check(lib().tg_debug_fill_lds(self._h, C.c_uint32(pattern)), "debug_fill_lds")

    def get_sim_params(self) -> abi.tg_sim_params:
        """gym.get_sim_params (vec_task.py:650): a copy of the live params."""
        sp = abi.tg_sim_params()
        check(lib().tg_get_sim_params(self._h, C.byref(sp)), "get_sim_params")
        return sp

    def set_sim_params(self, sp: abi.tg_sim_params):
        """gym.set_sim_params (vec_task.py:660), effective from the next simulate
        (substeps 0: simulate passes the state through, the recorded-physics replays)."""
        check(lib().tg_set_sim_params(self._h, C.byref(sp)), "set_sim_params")
        self.params = sp
        self.gravity = [float(x) for x in sp.gravity]

    def acquire_rigid_body_state_tensor(self) -> torch.Tensor:
        """gym.acquire_rigid_body_state_tensor: [N*L, 13] world link states
        (origin pos, quat xyzw, com linvel, angvel), links in model order;
        filled by refresh_rigid_body_state_tensor."""
        if getattr(self, "rigid_body_state", None) is None:
            self.rigid_body_state = torch.zeros(self.num_envs * self.L, 13, dtype=torch.float32, device=self.device)
        return self.rigid_body_state

    def refresh_rigid_body_state_tensor(self):
        rb = self.acquire_rigid_body_state_tensor()
        check(lib().tg_rigid_body_states(self._h, _ptr(rb)), "refresh_rigid_body_state_tensor")

    def acquire_net_contact_force_tensor(self) -> torch.Tensor:
        """gym.acquire_net_contact_force_tensor (tasks/anymal.py:113): [N, L, 3]
        live tensor, the ground's force on each link (world frame, newtons,
        links in model order) averaged over the last simulate's substeps;
        written by every simulate from now on.  Rows of links without a
        collision shape stay 0 (``contact_link_indices`` lists the others).
        Compiled-in models only; the task steps run unfused while it is on."""
        if getattr(self, "net_contact_force", None) is None:
            t = torch.zeros(self.num_envs, self.L, 3, dtype=torch.float32, device=self.device)
            check(lib().tg_set_net_contact_force_tensor(self._h, _ptr(t)), "acquire_net_contact_force_tensor")
            self.net_contact_force = t
        return self.net_contact_force

    def refresh_net_contact_force_tensor(self):
        """gym.refresh_net_contact_force_tensor (tasks/anymal.py:117): the tensor
        is written by simulate itself, nothing to do."""

    def acquire_dof_force_tensor(self) -> torch.Tensor:
        """gym.acquire_dof_force_tensor (tasks/MA_OP3.py:91): [N, D] live tensor,
        the actuator's force on each DOF (N m revolute, N prismatic) averaged
        over the last simulate's substeps: the implicit PD law at the stored
        end-of-substep velocity, +-effort where the clamp acted, the clamped
        actuation in effort mode, 0 for undriven and locked DOFs (tgsim.h);
        written by every simulate from now on.  No per-actor
        enable_actor_dof_force_sensors is needed.  Compiled-in models only;
        the task steps run unfused while it is on."""
        if getattr(self, "dof_force", None) is None:
            t = torch.zeros(self.num_envs, self.D, dtype=torch.float32, device=self.device)
            check(lib().tg_set_dof_force_tensor(self._h, _ptr(t)), "acquire_dof_force_tensor")
            self.dof_force = t
        return self.dof_force

    def refresh_dof_force_tensor(self):
        """gym.refresh_dof_force_tensor (tasks/MA_OP3.py:96): the tensor is
        written by simulate itself, nothing to do."""

    def acquire_force_sensor_tensor(self, sensors, space: str = "env") -> torch.Tensor:
        """gym.acquire_force_sensor_tensor (tasks/humanoid.py:167), with the
        sensors given here instead of through create_asset_force_sensor:
        ``sensors`` is a list of ``contact_frame(link, offset)`` (at most
        ``abi.TG_FS_MAX_SENSORS``; link names or indices stand for a frame at
        the link origin).  Returns the live [N, S, 6] tensor: per sensor the
        ground's force on the sensor's link and its moment about the sensor
        point (newtons, newton metres), averaged over the last simulate's
        substeps and written by every simulate from now on (tgsim.h
        tg_set_force_sensor_tensor).  ``space``: "env" for world axes, the
        convention of ``ContactDynamics.wrench``, or "local" for the link's own
        axes.  It is the ground reaction alone -- no gravity or inertial part,
        nothing from the links further down the chain -- and 0 for a link
        without collision shapes.  The same sensors and space again return the
        same tensor; other ones re-register and return a new tensor.  An empty
        ``sensors`` list turns the tensor off (``force_sensor`` is None again,
        the fused task steps are back) and returns an empty [N, 0, 6] tensor.
        Compiled-in models only; the task steps run unfused while it is on."""
        if space not in ("env", "local"):
            raise ValueError(f"space {space!r} is neither 'env' nor 'local'")
        sensors = [c if isinstance(c, abi.tg_contact_frame) else self.contact_frame(c) for c in sensors]
        key = (space, tuple((int(c.link), tuple(float(v) for v in c.offset)) for c in sensors))
        if self.force_sensor is not None and self._force_sensor_key == key:
            return self.force_sensor
        S = len(sensors)
        t = torch.zeros(self.num_envs, S, 6, dtype=torch.float32, device=self.device)
        frames = (abi.tg_contact_frame * max(S, 1))(*sensors)
        check(lib().tg_set_force_sensor_tensor(self._h, frames, S, abi.TG_LOCAL_SPACE if space == "local"
                                               else abi.TG_ENV_SPACE, _ptr(t) if S else None),
              "acquire_force_sensor_tensor")
        self.force_sensor = t if S else None
        self._force_sensor_key = key if S else None
        return t

    def refresh_force_sensor_tensor(self):
        """gym.refresh_force_sensor_tensor (tasks/humanoid.py:243): the tensor
        is written by simulate itself, nothing to do."""

    def acquire_jacobian_tensor(self) -> torch.Tensor:
        """gym.acquire_jacobian_tensor (tasks/gogoro/gogoro.py:108-114): the link
        Jacobians, filled by refresh_jacobian_tensors.  Floating base:
        [N, L, 6, D+6] -- J[e, l] maps u = (root com velocity, root angular
        velocity, qd) to link l's com linear velocity (rows 0..2) and angular
        velocity (rows 3..5), world frame, the rows of the rigid-body state
        tensor (tgsim.h tg_jacobians).  With fix_base, IsaacGym's rule: the
        view [N, L-1, 6, D] (no root link, no base columns) of the same
        storage."""
        if getattr(self, "_jacobian", None) is None:
            self._jacobian = torch.zeros(self.num_envs, self.L, 6, self.D + 6, dtype=torch.float32,
                                         device=self.device)
        return self._jacobian[:, 1:, :, 6:] if self.params.fix_base else self._jacobian

    def refresh_jacobian_tensors(self):
        """gym.refresh_jacobian_tensors (gogoro.py:396): one kernel launch from
        the current root and dof state, on the sim's stream."""
        self.acquire_jacobian_tensor()
        check(lib().tg_jacobians(self._h, _ptr(self._jacobian)), "refresh_jacobian_tensors")

    def acquire_mass_matrix_tensor(self) -> torch.Tensor:
        """gym.acquire_mass_matrix_tensor (tasks/franka_cube_stack.py:393): the
        joint-space inertia in the Jacobian's generalised velocity, filled by
        refresh_mass_matrix_tensors.  Floating base: [N, D+6, D+6], per-env
        mass scales and armature included (tgsim.h tg_mass_matrices); with
        fix_base the view [N, D, D] of the same storage."""
        if getattr(self, "_mass_matrix", None) is None:
            self._mass_matrix = torch.zeros(self.num_envs, self.D + 6, self.D + 6, dtype=torch.float32,
                                            device=self.device)
        return self._mass_matrix[:, 6:, 6:] if self.params.fix_base else self._mass_matrix

    def refresh_mass_matrix_tensors(self):
        """gym.refresh_mass_matrix_tensors (franka_cube_stack.py:441): one kernel
        launch from the current root and dof state, on the sim's stream."""
        self.acquire_mass_matrix_tensor()
        check(lib().tg_mass_matrices(self._h, _ptr(self._mass_matrix)), "refresh_mass_matrix_tensors")

    def _name_index(self, what: str, x) -> int:
        """index of a link / DOF given by name or index"""
        if isinstance(x, str):
            if what == "link":
                names = self.model.link_names if isinstance(self.model, NativeModel) else \
                    [l.name for l in self.model.links]
            else:
                names = self.model.dof_names
            if x not in names:
                raise KeyError(f"no {what} named {x!r}")
            return list(names).index(x)
        return int(x)

    def ik_chain(self, link, dofs=None, num_dofs=None, offset=(0.0, 0.0, 0.0)) -> abi.tg_ik_chain:
        """One chain of ``solve_ik`` (tgsim.h tg_ik_chain): the end-effector
        ``link`` and the ``dofs`` the solve may move, names or indices, at most
        8; ``offset`` is the controlled point in the link frame.  With
        ``dofs=None`` the chain is the DOFs on the path root -> link in that
        order, the last ``num_dofs`` of them (default: all, at most 8) -- the
        rider's arm of tasks/gogoro/gogoro.py:396-397 is
        ``ik_chain("r_arm_end_link", num_dofs=7)``."""
        d = self.desc.desc
        l = self._name_index("link", link)
        if not 0 <= l < self.L:
            raise ValueError(f"link {link!r} outside [0, {self.L})")
        if dofs is None:
            path, k = [], l
            while k >= 0:
                if d.link_dof[k] >= 0:
                    path.append(int(d.link_dof[k]))
                k = int(d.link_parent[k])
            path.reverse()
            keep = min(len(path), abi.TG_IK_MAX_DOFS) if num_dofs is None else int(num_dofs)
            if not 1 <= keep <= min(len(path), abi.TG_IK_MAX_DOFS):
                raise ValueError(f"num_dofs {num_dofs} outside 1..{min(len(path), abi.TG_IK_MAX_DOFS)} for link "
                                 f"{link!r} ({len(path)} DOFs on its path)")
            idx = path[len(path) - keep:]
        else:
            idx = [self._name_index("dof", x) for x in dofs]
            if num_dofs is not None and int(num_dofs) != len(idx):
                raise ValueError(f"num_dofs {num_dofs} does not match the {len(idx)} dofs given")
            if not 1 <= len(idx) <= abi.TG_IK_MAX_DOFS:
                raise ValueError(f"a chain takes 1..{abi.TG_IK_MAX_DOFS} DOFs, got {len(idx)}")
        c = abi.tg_ik_chain()
        c.link, c.num_dofs = l, len(idx)
        for i, x in enumerate(idx):
            c.dofs[i] = x
        c.offset[:] = [float(v) for v in offset]
        return c

    def solve_ik(self, chains, goal_pos: torch.Tensor, goal_quat: torch.Tensor | None = None, damping: float = 0.3,
                 targets: torch.Tensor | None = None, return_error: bool = False):
        """The hand IK of tasks/gogoro/gogoro.py:381-427 in one kernel launch
        (tgsim.h tg_ik_dls): for each of the K ``chains`` (``ik_chain``) the
        damped-least-squares step ``J^T (J J^T + damping^2 I)^-1 dpose``
        towards ``goal_pos`` [N, K, 3] and ``goal_quat`` [N, K, 4] (xyzw; None:
        position only), from the current root and dof state, on the sim's
        stream.  Returns ``dq`` [N, K, 8] (columns past a chain's DOFs are 0),
        with ``return_error`` also the pose error [N, K, 6]; both are owned by
        the sim and overwritten by the next call with as many chains.  With
        ``targets`` [N, D] (e.g. ``dof_pos_target``) the kernel also writes
        ``q + dq`` (summed over the chains that share a DOF) into the chain
        DOFs' columns and leaves the others alone."""
        chains = list(chains)
        K = len(chains)
        if not 1 <= K <= abi.TG_IK_MAX_CHAINS:
            raise ValueError(f"solve_ik takes 1..{abi.TG_IK_MAX_CHAINS} chains, got {K}")

        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        N = self.num_envs
        checked(goal_pos, (N, K, 3), "goal_pos")
        if goal_quat is not None:
            checked(goal_quat, (N, K, 4), "goal_quat")
        if targets is not None:
            checked(targets, (N, self.D), "targets")
        out = getattr(self, "_ik_out", None)
        if out is None:
            out = self._ik_out = {}
        if K not in out:
            out[K] = (torch.zeros(N, K, abi.TG_IK_MAX_DOFS, dtype=torch.float32, device=self.device),
                      torch.zeros(N, K, 6, dtype=torch.float32, device=self.device))
        dq, err = out[K]
        arr = (abi.tg_ik_chain * K)(*chains)
        check(lib().tg_ik_dls(self._h, arr, K, _ptr(goal_pos), _ptr(goal_quat), float(damping), _ptr(dq), _ptr(err),
                              _ptr(targets)), "solve_ik")
        return (dq, err) if return_error else dq

    def solve_osc(self, chains, goal_pos: torch.Tensor, goal_quat: torch.Tensor | None = None, kp: float = 150.0,
                  kd: float | None = None, kp_null: float = 10.0, kd_null: float | None = None,
                  q_rest: torch.Tensor | None = None, damping: float = 1e-2, efforts: torch.Tensor | None = None,
                  return_error: bool = False):
        """Operational-space control, _compute_osc_torques of
        tasks/franka_cube_stack.py:602-628, in one kernel launch (tgsim.h
        tg_osc): for each of the K ``chains`` (``ik_chain``) the joint torques
        ``J^T Lambda (kp err - kd v)`` that pull the chain's controlled point
        towards ``goal_pos`` [N, K, 3] and ``goal_quat`` [N, K, 4] (xyzw; None:
        position only), ``Lambda = (J H_c^-1 J^T + damping^2 I)^-1`` with the
        chain's own block ``H_c`` of the mass matrix, from the current state,
        on the sim's stream.  ``kd`` and ``kd_null`` default to
        ``2 sqrt(kp)`` and ``2 sqrt(kp_null)``, the reference's.  With
        ``q_rest`` [N, D] the null-space term that draws the chain's joints to
        ``q_rest`` without accelerating the point is added.  Returns ``tau``
        [N, K, 8] (columns past a chain's DOFs are 0, not clamped), with
        ``return_error`` also the pose error [N, K, 6]; both are owned by the
        sim and overwritten by the next call with as many chains.  With
        ``efforts`` [N, D] (e.g. ``dof_actuation``) the kernel also writes the
        torques, summed over the chains that share a DOF and clamped to the
        DOF's effort limit, into the chain DOFs' columns and leaves the others
        alone."""
        chains = list(chains)
        K = len(chains)
        if not 1 <= K <= abi.TG_IK_MAX_CHAINS:
            raise ValueError(f"solve_osc takes 1..{abi.TG_IK_MAX_CHAINS} chains, got {K}")

        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        N = self.num_envs
        checked(goal_pos, (N, K, 3), "goal_pos")
        if goal_quat is not None:
            checked(goal_quat, (N, K, 4), "goal_quat")
        if q_rest is not None:
            checked(q_rest, (N, self.D), "q_rest")
        if efforts is not None:
            checked(efforts, (N, self.D), "efforts")
        kd = 2.0 * float(kp) ** 0.5 if kd is None else kd
        kd_null = 2.0 * float(kp_null) ** 0.5 if kd_null is None else kd_null
        gains = abi.tg_osc_gains(float(kp), float(kd), float(kp_null), float(kd_null), float(damping))
        out = getattr(self, "_osc_out", None)
        if out is None:
            out = self._osc_out = {}
        if K not in out:
            out[K] = (torch.zeros(N, K, abi.TG_IK_MAX_DOFS, dtype=torch.float32, device=self.device),
                      torch.zeros(N, K, 6, dtype=torch.float32, device=self.device))
        tau, err = out[K]
        arr = (abi.tg_ik_chain * K)(*chains)
        check(lib().tg_osc(self._h, arr, K, _ptr(goal_pos), _ptr(goal_quat), _ptr(q_rest), C.byref(gains), _ptr(tau),
                           _ptr(err), _ptr(efforts)), "solve_osc")
        return (tau, err) if return_error else tau

    def inverse_dynamics(self, accel: torch.Tensor | None = None, gravity: bool = True, velocity: bool = True,
                         dofs=None, efforts: torch.Tensor | None = None, accumulate: bool = False,
                         out: torch.Tensor | None = None) -> torch.Tensor:
        """Inverse dynamics in one kernel launch (tgsim.h tg_inverse_dynamics):
        ``tau = H a + h(q, u)`` [N, 6 + D] in the coordinates of the Jacobian
        and mass-matrix tensors, from the current state, the sim's gravity, the
        body mass scales and the armature, on the sim's stream.  ``gravity``
        and ``velocity`` switch the two parts of the bias force ``h`` -- the
        weight and the Coriolis / centrifugal terms; ``accel`` [N, 6 + D]
        (None: 0) is the acceleration ``a``.  ``tau[:, :3]`` is the net force,
        ``tau[:, 3:6]`` the net moment about the root link's centre of mass,
        ``tau[:, 6 + d]`` DOF d's generalised force.  Returns ``out`` if given,
        else a tensor owned by the sim that the next call overwrites.  With
        ``efforts`` [N, D] (e.g. ``dof_actuation``) the kernel also writes DOF
        d's entry, clamped to the DOF's effort limit, for every DOF in ``dofs``
        (names or indices; None: all) and leaves the others alone; with
        ``accumulate`` it adds to what ``efforts`` holds before it clamps --
        after ``solve_osc(..., efforts=sim.dof_actuation)`` this is gravity and
        Coriolis compensation of the controlled chains (clamped twice)."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        N, C_ = self.num_envs, 6 + self.D
        if accel is not None:
            checked(accel, (N, C_), "accel")
        if efforts is not None:
            checked(efforts, (N, self.D), "efforts")
        if out is not None:
            checked(out, (N, C_), "out")
        else:
            out = getattr(self, "_id_out", None)
            if out is None:
                out = self._id_out = torch.zeros(N, C_, dtype=torch.float32, device=self.device)
        terms = (abi.TG_ID_GRAVITY if gravity else 0) | (abi.TG_ID_VELOCITY if velocity else 0)
        if terms == 0 and accel is None:
            raise ValueError("inverse_dynamics without gravity, velocity and accel has nothing to compute")
        idx = [] if dofs is None else [self._name_index("dof", x) for x in dofs]
        if dofs is not None and not idx:
            raise ValueError("dofs is empty; pass None for every DOF")
        arr = (C.c_int32 * len(idx))(*idx) if idx else None
        check(lib().tg_inverse_dynamics(self._h, terms, _ptr(accel), _ptr(out), _ptr(efforts), arr, len(idx),
                                        1 if accumulate else 0), "inverse_dynamics")
        return out

    def contact_frame(self, link, offset=(0.0, 0.0, 0.0)) -> abi.tg_contact_frame:
        """One contact of ``contact_inverse_dynamics`` (tgsim.h
        tg_contact_frame): the ``link`` in contact, by name or index, and the
        contact point ``offset`` in the link frame (the convention of
        ``ik_chain``)."""
        l = self._name_index("link", link)
        if not 0 <= l < self.L:
            raise ValueError(f"link {link!r} outside [0, {self.L})")
        c = abi.tg_contact_frame()
        c.link = l
        c.offset[:] = [float(v) for v in offset]
        return c

    def contact_inverse_dynamics(self, contacts, share: torch.Tensor | None = None, accel: torch.Tensor | None = None,
                                 gravity: bool = True, velocity: bool = True, moment_arm: float = 0.1,
                                 out: torch.Tensor | None = None, wrench: torch.Tensor | None = None, dofs=None,
                                 efforts: torch.Tensor | None = None,
                                 accumulate: bool = False) -> "ContactDynamics":
        """Inverse dynamics of the floating-base robot standing on the K
        ``contacts`` (``contact_frame``, at most 4), in one kernel launch
        (tgsim.h tg_contact_inverse_dynamics).  With ``b = H a + h`` exactly
        what ``inverse_dynamics`` returns for the same ``accel``, ``gravity``
        and ``velocity``, the base rows ``b[:, :6]`` are distributed over the
        contacts as the wrenches (force, moment about the contact point; world
        axes, acting on the robot) of least cost ``sum_k (|f_k|^2 + |n_k|^2 /
        moment_arm^2) / share_k`` -- a least-squares distribution that knows
        nothing of unilateral contact, friction cones or the foot's outline;
        judge the returned wrenches and steer them with ``share`` [N, K] (None:
        ones; 0 unloads a contact exactly, a swing foot; an env with all zeros
        is airborne and gets the plain inverse dynamics).  Returns
        ``ContactDynamics(tau, wrench)``: ``tau`` [N, 6 + D] with the joint
        torques that are left in ``tau[:, 6:]`` and the base wrench the
        contacts do not carry (0 up to rounding) in ``tau[:, :6]``, ``wrench``
        [N, K, 6].  They are ``out`` / ``wrench`` if given, else tensors owned
        by the sim that the next call (with as many contacts) overwrites.
        ``efforts``, ``dofs`` and ``accumulate`` as in ``inverse_dynamics``:
        ``contact_inverse_dynamics(feet, efforts=sim.dof_actuation)`` is
        gravity compensation of the standing robot."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        contacts = list(contacts)
        K = len(contacts)
        if not 1 <= K <= abi.TG_CID_MAX_CONTACTS:
            raise ValueError(f"contact_inverse_dynamics takes 1..{abi.TG_CID_MAX_CONTACTS} contacts, got {K}")
        contacts = [c if isinstance(c, abi.tg_contact_frame) else self.contact_frame(c) for c in contacts]
        N, C_ = self.num_envs, 6 + self.D
        for t, shape, what in ((share, (N, K), "share"), (accel, (N, C_), "accel"), (efforts, (N, self.D), "efforts"),
                               (out, (N, C_), "out"), (wrench, (N, K, 6), "wrench")):
            if t is not None:
                checked(t, shape, what)
        own = getattr(self, "_cid_out", None)
        if own is None:
            own = self._cid_out = {}
        if out is None:
            if "tau" not in own:
                own["tau"] = torch.zeros(N, C_, dtype=torch.float32, device=self.device)
            out = own["tau"]
        if wrench is None:
            if K not in own:
                own[K] = torch.zeros(N, K, 6, dtype=torch.float32, device=self.device)
            wrench = own[K]
        terms = (abi.TG_ID_GRAVITY if gravity else 0) | (abi.TG_ID_VELOCITY if velocity else 0)
        if terms == 0 and accel is None:
            raise ValueError("contact_inverse_dynamics without gravity, velocity and accel has nothing to compute")
        idx = [] if dofs is None else [self._name_index("dof", x) for x in dofs]
        if dofs is not None and not idx:
            raise ValueError("dofs is empty; pass None for every DOF")
        arr = (C.c_int32 * len(idx))(*idx) if idx else None
        frames = (abi.tg_contact_frame * K)(*contacts)
        check(lib().tg_contact_inverse_dynamics(self._h, frames, K, _ptr(share), float(moment_arm), terms, _ptr(accel),
                                                _ptr(out), _ptr(wrench), _ptr(efforts), arr, len(idx),
                                                1 if accumulate else 0), "contact_inverse_dynamics")
        return ContactDynamics(out, wrench)

    def contact_qp(self, contacts, extents, mu: float = 0.7, friction: torch.Tensor | None = None,
                   normals: torch.Tensor | None = None, share: torch.Tensor | None = None,
                   accel: torch.Tensor | None = None, gravity: bool = True, velocity: bool = True,
                   moment_arm: float = 0.1, reg: float = abi.TG_QP_DEFAULTS["reg"],
                   rho: float = abi.TG_QP_DEFAULTS["rho"], relax: float = abi.TG_QP_DEFAULTS["relax"],
                   iters: int = abi.TG_QP_DEFAULTS["iters"], forces: bool = False, info: bool = False,
                   efforts: torch.Tensor | None = None, dofs=None, accumulate: bool = False) -> "ContactForces":
        """``contact_inverse_dynamics`` with contact forces the ground can
        supply, in one kernel launch (tgsim.h tg_contact_qp).  Each of the K
        ``contacts`` (``contact_frame``, at most 4) is a rectangular patch with
        half extents ``extents[k] = (hx, hy)`` in the link's x and y axes about
        the frame's offset ((0, 0): a point); ``walk_sole_patch`` gives a foot's.
        The forces at the 4 K patch vertices are confined to the friction cone
        of their contact -- normal ``normals`` [N, K, 3] (None: world z; e.g.
        ``height_scan(normals=True)``), coefficient ``friction`` [N, K] or the
        scalar ``mu`` -- and come as near to balancing the base rows of ``b = H
        a + h`` as the cones allow, by ``iters`` iterations of the header's ADMM
        (``reg``, ``rho``, ``relax``), every returned force feasible after any
        number of them.  ``share`` [N, K] weighs the contacts (0 removes one
        exactly).  Returns ``ContactForces(tau, wrench, forces, info)``:
        ``tau`` [N, 6 + D] with the joint torques in ``tau[:, 6:]`` and the
        base wrench the ground cannot supply in ``tau[:, :6]``; ``wrench`` [N,
        K, 6] (force, moment about the contact point) in the convention of
        ``contact_inverse_dynamics``; with ``forces`` the vertex forces [N, K,
        4, 3]; with ``info`` [N, 4]: ``|tau[:3]|``, ``|tau[3:6]|``, the last
        iteration's ``max |x - z|`` and the number of loaded vertices; a part
        not requested is None.  The tensors are owned by the sim and
        overwritten by the next call with as many contacts.  ``accel``,
        ``gravity``, ``velocity``, ``moment_arm``, ``efforts``, ``dofs`` and
        ``accumulate`` as in ``contact_inverse_dynamics``."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        contacts = list(contacts)
        K = len(contacts)
        if not 1 <= K <= abi.TG_CID_MAX_CONTACTS:
            raise ValueError(f"contact_qp takes 1..{abi.TG_CID_MAX_CONTACTS} contacts, got {K}")
        contacts = [c if isinstance(c, abi.tg_contact_frame) else self.contact_frame(c) for c in contacts]
        ext = [tuple(float(v) for v in x) for x in extents]
        if len(ext) != K or any(len(x) != 2 for x in ext):
            raise ValueError(f"extents must be {K} pairs (hx, hy), got {extents!r}")
        N, C_ = self.num_envs, 6 + self.D
        for t, shape, what in ((friction, (N, K), "friction"), (normals, (N, K, 3), "normals"), (share, (N, K), "share"),
                               (accel, (N, C_), "accel"), (efforts, (N, self.D), "efforts")):
            if t is not None:
                checked(t, shape, what)
        own = getattr(self, "_qp_out", None)
        if own is None:
            own = self._qp_out = {}

        def owned(key, shape):
            if key not in own:
                own[key] = torch.zeros(*shape, dtype=torch.float32, device=self.device)
            return own[key]

        tau, wrench = owned("tau", (N, C_)), owned(("wrench", K), (N, K, 6))
        fo = owned(("forces", K), (N, K, 4, 3)) if forces else None
        io = owned("info", (N, 4)) if info else None
        terms = (abi.TG_ID_GRAVITY if gravity else 0) | (abi.TG_ID_VELOCITY if velocity else 0)
        if terms == 0 and accel is None:
            raise ValueError("contact_qp without gravity, velocity and accel has nothing to compute")
        idx = [] if dofs is None else [self._name_index("dof", x) for x in dofs]
        if dofs is not None and not idx:
            raise ValueError("dofs is empty; pass None for every DOF")
        arr = (C.c_int32 * len(idx))(*idx) if idx else None
        frames = (abi.tg_contact_frame * K)(*contacts)
        hxy = (C.c_float * (2 * K))(*[v for x in ext for v in x])
        check(lib().tg_contact_qp(self._h, frames, K, hxy, _ptr(normals), _ptr(friction), float(mu), _ptr(share),
                                  float(moment_arm), float(reg), float(rho), float(relax), int(iters), terms,
                                  _ptr(accel), _ptr(tau), _ptr(wrench), _ptr(fo), _ptr(io), _ptr(efforts), arr,
                                  len(idx), 1 if accumulate else 0), "contact_qp")
        return ContactForces(tau, wrench, fo, io)

    def centroidal(self, matrix: bool = False, bias: bool = False, out: torch.Tensor | None = None,
                   out_matrix: torch.Tensor | None = None, out_bias: torch.Tensor | None = None) -> "Centroidal":
        """Centroidal quantities in one kernel launch (tgsim.h tg_centroidal),
        from the current state and the body mass scales, on the sim's stream.
        Returns ``Centroidal(state, matrix, bias)``.  ``state`` [N, 16]: the
        whole-body centre of mass ``[0:3]`` (world), its velocity ``[3:6]``,
        the angular momentum about it ``[6:9]``, the total mass ``[9]`` and the
        centroidal inertia ``[10:16]`` (xx yy zz xy xz yz).  With ``matrix``
        the centroidal momentum matrix ``A`` [N, 6, 6 + D] in the columns of
        the Jacobian tensor, ``A u = (M c', k)``, ``A[:, :3] / M`` the CoM
        Jacobian; with ``bias`` the momentum rate ``A' u`` [N, 6] at ``u' = 0``
        without gravity.  A part that was not requested is None and costs
        nothing.  ``out``, ``out_matrix`` and ``out_bias`` are checked and, for
        a requested part, written and returned as given; an ``out_matrix`` or
        ``out_bias`` passed without ``matrix`` / ``bias`` is left untouched.
        Without them the tensors are owned by the sim and overwritten by the
        next call."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        def own(key, shape):
            buf = getattr(self, "_centroidal_out", None)
            if buf is None:
                buf = self._centroidal_out = {}
            if key not in buf:
                buf[key] = torch.zeros(*shape, dtype=torch.float32, device=self.device)
            return buf[key]

        N = self.num_envs
        shapes = {"out": (N, abi.TG_CENTROIDAL_STATE), "out_matrix": (N, 6, 6 + self.D), "out_bias": (N, 6)}
        given = {"out": out, "out_matrix": out_matrix, "out_bias": out_bias}
        for key, t in given.items():
            if t is not None:
                checked(t, shapes[key], key)
        st, mt, bt = ((given[key] if given[key] is not None else own(key, shapes[key])) if asked else None
                      for key, asked in (("out", True), ("out_matrix", matrix), ("out_bias", bias)))
        check(lib().tg_centroidal(self._h, _ptr(st), _ptr(mt), _ptr(bt)), "centroidal")
        return Centroidal(st, mt, bt)

    def scan_grid(self, xs, ys) -> torch.Tensor:
        """The pattern ``[len(xs) * len(ys), 2]`` of ``height_scan`` over the
        grid ``xs`` x ``ys`` (metres, in the frame's axes), float32 on the
        sim's device, in the order of the reference's ``init_height_points``
        (tasks/anymal_terrain.py:501-511): ``torch.meshgrid(x, y)`` with ij
        indexing, flattened -- x varies slowest."""
        x = torch.as_tensor(xs, dtype=torch.float32).reshape(-1)
        y = torch.as_tensor(ys, dtype=torch.float32).reshape(-1)
        gx, gy = torch.meshgrid(x, y, indexing="ij")
        return torch.stack([gx.reshape(-1), gy.reshape(-1)], dim=1).contiguous().to(self.device)

    def height_scan(self, frames, points: torch.Tensor, surface: str = "surface", align: str = "yaw",
                    normals: bool = False, relative: dict | None = None, out: torch.Tensor | None = None,
                    out_normals: torch.Tensor | None = None) -> "HeightScan":
        """The ground under the robot in one kernel launch (tgsim.h
        tg_height_scan), from the current state and the sim's heightfield, on
        the sim's stream.  ``frames``: 1..8 ``contact_frame`` (a link, by name
        or index, stands for its origin); ``points`` [P, 2] float32 on the
        sim's device (``scan_grid``), one pattern for every env and frame,
        P <= 1024.  Sample k of frame f lies at the frame point's world x, y
        plus ``points[k]`` turned by the link's heading (``align="yaw"``, the
        reference's ``quat_apply_yaw``), not at all (``"world"``), or laid out
        in the link's own axes and dropped vertically (``"link"``).
        ``surface="surface"`` reads the surface the contacts feel -- the
        heightfield's triangles or the z = 0 plane, whichever is higher -- and
        ``"cell"`` the reference's ``get_heights`` rule, the lower of two
        corners of the cell (it has no normals).  Returns ``HeightScan(heights,
        normals)``: ``heights`` [N, F, P]; with ``normals`` the unit surface
        normals [N, F, P, 3], else None.  ``relative=dict(bias=, lo=, hi=,
        scale=)`` turns the heights into ``clamp(p_f.z - bias - h, lo, hi) *
        scale``, the reference's height observation (bias 0.5, -1, 1,
        heightMeasurementScale) or a foot's clearance.  ``out`` and
        ``out_normals`` are checked and, for a requested part, written and
        returned as given; without them the tensors are owned by the sim and
        overwritten by the next call with as many frames and points."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        def own(key, shape):
            buf = getattr(self, "_scan_out", None)
            if buf is None:
                buf = self._scan_out = {}
            if (key, shape) not in buf:
                buf[key, shape] = torch.zeros(*shape, dtype=torch.float32, device=self.device)
            return buf[key, shape]

        rules = {"surface": abi.TG_SCAN_SURFACE, "cell": abi.TG_SCAN_CELL}
        aligns = {"yaw": abi.TG_SCAN_YAW, "world": abi.TG_SCAN_WORLD, "link": abi.TG_SCAN_LINK}
        if surface not in rules:
            raise ValueError(f"surface must be one of {sorted(rules)}, got {surface!r}")
        if align not in aligns:
            raise ValueError(f"align must be one of {sorted(aligns)}, got {align!r}")
        if normals and surface == "cell":
            raise ValueError("the cell rule has no normals")
        frames = [c if isinstance(c, abi.tg_contact_frame) else self.contact_frame(c) for c in frames]
        F = len(frames)
        if not 1 <= F <= abi.TG_SCAN_MAX_FRAMES:
            raise ValueError(f"height_scan takes 1..{abi.TG_SCAN_MAX_FRAMES} frames, got {F}")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 2:
            raise ValueError("points must be a [P, 2] tensor")
        P = int(points.shape[0])
        if not 1 <= P <= abi.TG_SCAN_MAX_POINTS:
            raise ValueError(f"height_scan takes 1..{abi.TG_SCAN_MAX_POINTS} points, got {P}")
        checked(points, (P, 2), "points")
        N = self.num_envs
        shapes = {"out": (N, F, P), "out_normals": (N, F, P, 3)}
        given = {"out": out, "out_normals": out_normals}
        for key, t in given.items():
            if t is not None:
                checked(t, shapes[key], key)
        ht, nt = ((given[key] if given[key] is not None else own(key, shapes[key])) if asked else None
                  for key, asked in (("out", True), ("out_normals", normals)))
        sp = abi.tg_scan_params()
        sp.surface, sp.align, sp.relative = rules[surface], aligns[align], 0
        if relative is not None:
            if set(relative) != {"bias", "lo", "hi", "scale"}:
                raise ValueError("relative must be dict(bias=, lo=, hi=, scale=)")
            sp.relative = 1
            sp.bias, sp.lo, sp.hi, sp.scale = (float(relative[k]) for k in ("bias", "lo", "hi", "scale"))
        arr = (abi.tg_contact_frame * F)(*frames)
        check(lib().tg_height_scan(self._h, arr, F, _ptr(points), P, C.byref(sp), _ptr(ht), _ptr(nt)), "height_scan")
        self._keep_scan_points = points   # read on the sim stream; held until the next call
        return HeightScan(ht, nt)

    def imu_history(self, num_sensors: int) -> torch.Tensor:
        """A fresh history tensor for ``imu``: zeros [N, num_sensors, 8] on the
        sim's device.  Its flag is 0, so the first reading comes out with
        ``valid = 0``."""
        S = int(num_sensors)
        if not 1 <= S <= abi.TG_IMU_MAX_SENSORS:
            raise ValueError(f"imu takes 1..{abi.TG_IMU_MAX_SENSORS} sensors, got {S}")
        return torch.zeros(self.num_envs, S, abi.TG_IMU_HISTORY, dtype=torch.float32, device=self.device)

    def imu(self, sensors, history: torch.Tensor | None = None, dt: float | None = None,
            reset: torch.Tensor | None = None, bias: torch.Tensor | None = None, gyro_noise: float = 0.0,
            accel_noise: float = 0.0, seed: int = 0, counter: int = 0, out: torch.Tensor | None = None) -> "Imu":
        """Inertial measurement units in one kernel launch (tgsim.h tg_imu), from
        the current state and the sim's gravity, on the sim's stream.
        ``sensors``: 1..8 ``contact_frame`` (a link, by name or index, stands
        for its origin); the sensor's axes are the link's.  Returns the named
        tuple ``Imu(quat, gravity, lin_vel, ang_vel, lin_acc, ang_acc, valid,
        raw)`` of views of ``raw`` [N, S, 20]: the link's world quaternion xyzw,
        the unit gravity direction, the sensor point's velocity, the gyro
        reading, the accelerometer reading (the specific force: ``+|g|`` along
        world up at rest, 0 in free fall) and the angular acceleration, all in
        the link's axes, and ``valid`` [N, S], 1.0 where the accelerations were
        differenced.  ``history`` [N, S, 8] (``imu_history``) is owned by the
        caller: it holds the world velocities of the previous call, which the
        accelerations are differenced against over ``dt`` -- the sim time since
        that call, by default the sim params' ``dt``, one ``simulate`` -- and
        is rewritten by this call.  Without a history, with a fresh one, and for
        the envs flagged in ``reset`` ([N] int64, a ``reset_buf``), the
        accelerations are 0, ``valid`` is 0 and the accelerometer reads
        ``-R^T g``.  ``bias`` [N, S, 6] is added to the gyro (0:3) and
        accelerometer (3:6) readings, and ``gyro_noise`` / ``accel_noise`` are
        the sigmas of Gaussian noise on them, the Philox draws of ``tg_rng_fill``
        kind 2 for (``seed``, ``counter``): pass a new ``counter`` every call.
        ``out`` is checked, written and returned as ``raw``; without it the
        tensor is owned by the sim and overwritten by the next call with as
        many sensors."""
        def checked(t, shape, what, dtype=torch.float32):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a {str(dtype).split('.')[-1]} tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        sensors = [c if isinstance(c, abi.tg_contact_frame) else self.contact_frame(c) for c in sensors]
        S = len(sensors)
        if not 1 <= S <= abi.TG_IMU_MAX_SENSORS:
            raise ValueError(f"imu takes 1..{abi.TG_IMU_MAX_SENSORS} sensors, got {S}")
        N = self.num_envs
        if history is not None:
            checked(history, (N, S, abi.TG_IMU_HISTORY), "history")
        if reset is not None:
            checked(reset, (N,), "reset", torch.int64)
        if bias is not None:
            checked(bias, (N, S, 6), "bias")
        if out is not None:
            raw = checked(out, (N, S, abi.TG_IMU_WIDTH), "out")
        else:
            buf = getattr(self, "_imu_out", None)
            if buf is None:
                buf = self._imu_out = {}
            if S not in buf:
                buf[S] = torch.zeros(N, S, abi.TG_IMU_WIDTH, dtype=torch.float32, device=self.device)
            raw = buf[S]
        ip = abi.tg_imu_params()
        ip.dt = float(self.params.dt if dt is None else dt)
        ip.gyro_noise, ip.accel_noise = float(gyro_noise), float(accel_noise)
        ip.seed, ip.counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
        arr = (abi.tg_contact_frame * S)(*sensors)
        check(lib().tg_imu(self._h, arr, S, C.byref(ip), _ptr(bias), _ptr(reset), _ptr(history), _ptr(raw)), "imu")
        self._keep_imu = (bias, reset)   # read on the sim stream; held until the next call
        # the views of the last raw tensor are kept: a task reads into the same one every step
        views = getattr(self, "_imu_views", None)
        if views is None or views.raw is not raw:
            views = self._imu_views = Imu(raw[..., 0:4], raw[..., 4:7], raw[..., 7:10], raw[..., 10:13],
                                          raw[..., 13:16], raw[..., 16:19], raw[..., 19], raw)
        return views

    def lidar_rays(self, azimuths, elevations) -> torch.Tensor:
        """The pattern ``[len(elevations) * len(azimuths), 6]`` of ``ray_cast``
        for a lidar: unit directions ``(cos e cos a, cos e sin a, sin e)``
        (radians; x forward, y left, z up), starts zero, elevation-major -- the
        azimuth varies fastest, one ring after the other.  float32 on the
        sim's device; with unit directions ``dist`` is the range."""
        a = torch.as_tensor(azimuths, dtype=torch.float64).reshape(-1)
        e = torch.as_tensor(elevations, dtype=torch.float64).reshape(-1)
        ee, aa = torch.meshgrid(e, a, indexing="ij")
        d = torch.stack([torch.cos(ee) * torch.cos(aa), torch.cos(ee) * torch.sin(aa), torch.sin(ee)], dim=-1)
        rays = torch.cat([torch.zeros_like(d), d], dim=-1).reshape(-1, 6)
        return rays.to(torch.float32).contiguous().to(self.device)

    def pinhole_rays(self, width: int, height: int, hfov: float) -> torch.Tensor:
        """The pattern ``[height * width, 6]`` of ``ray_cast`` for a pinhole
        depth camera looking along x (y left, z up) with the horizontal field
        of view ``hfov`` (radians) and square pixels: row-major from the
        top-left pixel, pixel (r, c) has the direction ``(1, T (1 - 2 (c + 1/2)
        / W), T (H / W) (1 - 2 (r + 1/2) / H))``, ``T = tan(hfov / 2)``, starts
        zero.  The directions are scaled to ``d.x = 1``, not to unit length, so
        that ``dist`` is the depth along the optical axis and ``max_range``
        bounds the depth.  float32 on the sim's device."""
        W, H = int(width), int(height)
        if W < 1 or H < 1 or not 0.0 < float(hfov) < math.pi:
            raise ValueError("pinhole_rays needs width, height >= 1 and 0 < hfov < pi")
        T = math.tan(0.5 * float(hfov))
        c = torch.arange(W, dtype=torch.float64)
        r = torch.arange(H, dtype=torch.float64)
        rr, cc = torch.meshgrid(r, c, indexing="ij")
        d = torch.stack([torch.ones_like(cc), T * (1.0 - 2.0 * (cc + 0.5) / W),
                         T * (H / W) * (1.0 - 2.0 * (rr + 0.5) / H)], dim=-1)
        rays = torch.cat([torch.zeros_like(d), d], dim=-1).reshape(-1, 6)
        return rays.to(torch.float32).contiguous().to(self.device)

    def ray_cast(self, frames, rays: torch.Tensor, align: str = "link", max_range: float = 20.0,
                 normals: bool = False, out: torch.Tensor | None = None,
                 out_normals: torch.Tensor | None = None) -> "RayCast":
        """Lidar and depth-camera ranges in one kernel launch (tgsim.h
        tg_ray_cast), from the current state and the sim's heightfield, on the
        sim's stream.  ``frames``: 1..8 ``contact_frame`` (a link, by name or
        index, stands for its origin); ``rays`` [R, 6] float32 on the sim's
        device (``lidar_rays``, ``pinhole_rays``), a start offset and a
        direction per ray, one pattern for every env and frame, R <= 4096.  The
        pattern is given in the link's own axes (``align="link"``), in axes
        turned by the link's heading only (``"yaw"``, ``height_scan``'s rule)
        or in world axes (``"world"``).  Ray k of frame f is ``x(t) = p_f + A
        s_k + t A d_k``; it is cast against the ground the contacts feel -- the
        solid under the heightfield's triangles and the z <= 0 half-space.
        Returns ``RayCast(dist, normals)``: ``dist`` [N, F, R], the smallest
        ``t`` in ``[0, max_range]`` at which the ray is in the ground
        (directions are not normalised: the range for unit directions, the
        depth for ``pinhole_rays``), and exactly ``max_range`` on a miss; with
        ``normals`` the unit normal of what was hit [N, F, R, 3] (zero on a
        miss), else None.  ``out`` and ``out_normals`` are checked and, for a
        requested part, written and returned as given; without them the tensors
        are owned by the sim and overwritten by the next call with as many
        frames and rays."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        def own(key, shape):
            buf = getattr(self, "_ray_out", None)
            if buf is None:
                buf = self._ray_out = {}
            if (key, shape) not in buf:
                buf[key, shape] = torch.zeros(*shape, dtype=torch.float32, device=self.device)
            return buf[key, shape]

        aligns = {"link": abi.TG_RAY_LINK, "yaw": abi.TG_RAY_YAW, "world": abi.TG_RAY_WORLD}
        if align not in aligns:
            raise ValueError(f"align must be one of {sorted(aligns)}, got {align!r}")
        max_range = float(max_range)
        if not (math.isfinite(max_range) and max_range > 0.0):
            raise ValueError(f"max_range must be a finite number > 0, got {max_range}")
        frames = [c if isinstance(c, abi.tg_contact_frame) else self.contact_frame(c) for c in frames]
        F = len(frames)
        if not 1 <= F <= abi.TG_RAY_MAX_FRAMES:
            raise ValueError(f"ray_cast takes 1..{abi.TG_RAY_MAX_FRAMES} frames, got {F}")
        if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 6:
            raise ValueError("rays must be a [R, 6] tensor")
        R = int(rays.shape[0])
        if not 1 <= R <= abi.TG_RAY_MAX_RAYS:
            raise ValueError(f"ray_cast takes 1..{abi.TG_RAY_MAX_RAYS} rays, got {R}")
        checked(rays, (R, 6), "rays")
        N = self.num_envs
        shapes = {"out": (N, F, R), "out_normals": (N, F, R, 3)}
        given = {"out": out, "out_normals": out_normals}
        for key, t in given.items():
            if t is not None:
                checked(t, shapes[key], key)
        dt, nt = ((given[key] if given[key] is not None else own(key, shapes[key])) if asked else None
                  for key, asked in (("out", True), ("out_normals", normals)))
        rp = abi.tg_ray_params()
        rp.align, rp.max_range = aligns[align], max_range
        arr = (abi.tg_contact_frame * F)(*frames)
        check(lib().tg_ray_cast(self._h, arr, F, _ptr(rays), R, C.byref(rp), _ptr(dt), _ptr(nt)), "ray_cast")
        self._keep_rays = rays   # read on the sim stream; held until the next call
        return RayCast(dt, nt)

    def capsule(self, link, p0, p1=None, radius: float = 0.05) -> abi.tg_capsule:
        """One capsule of ``proximity`` (tgsim.h tg_capsule): the ``link`` it is
        fixed to, by name or index, the end points ``p0`` and ``p1`` of its axis
        in the link frame (``p1=None``: a sphere about ``p0``) and its
        ``radius``."""
        l = self._name_index("link", link)
        if not 0 <= l < self.L:
            raise ValueError(f"link {link!r} outside [0, {self.L})")
        return make_capsule(l, p0, p1, radius)

    def limb_capsule(self, link, child, radius: float) -> abi.tg_capsule:
        """The capsule of the limb segment ``link``: from the link's origin to the
        origin of the joint that carries ``child``, in the link frame -- the
        thigh is ``limb_capsule("l_leg_hip_p_link", "l_leg_kn_p_link", r)``.
        Raises if ``child``'s parent is not ``link``."""
        parent, origin = link_tree(self.desc)
        l, c = self._name_index("link", link), self._name_index("link", child)
        if not (0 <= l < self.L and 0 <= c < self.L):
            raise ValueError(f"links {link!r}, {child!r} outside [0, {self.L})")
        return limb_capsule(parent, origin, l, c, radius)

    def capsule_pairs(self, capsules, min_hops: int = 3) -> list:
        """Every pair ``(a, b)``, ``a < b``, of ``capsules`` whose links are at
        least ``min_hops`` joints apart in the link tree, in increasing order:
        with the default, capsules on the same link, on a parent and its child
        and on a grandparent and its grandchild (or two siblings) are left
        out -- neighbours along a limb overlap by construction.  Raises above
        256 pairs (tgsim.h TG_PROX_MAX_PAIRS)."""
        return capsule_pairs(link_tree(self.desc)[0], capsules, min_hops)

    def proximity(self, capsules, pairs, margin: float = 0.0, dist: bool = True, witness: bool = False,
                  summary: bool = False, out: torch.Tensor | None = None, out_witness: torch.Tensor | None = None,
                  out_summary: torch.Tensor | None = None) -> "Proximity":
        """Capsule distances between the robot's own links in one kernel launch
        (tgsim.h tg_proximity), from the current state, on the sim's stream.
        ``capsules``: 1..32 ``capsule`` / ``limb_capsule``; ``pairs``: 1..256
        pairs of indices into them (``capsule_pairs``).  Returns the named tuple
        ``Proximity(dist, witness, summary)``, each None unless asked for:
        ``dist`` [N, P], the distance between the two axis segments less the
        two radii, negative by the penetration depth; ``witness`` [N, P, 6], a
        closest point on the first axis and one on the second, world
        coordinates; ``summary`` [N, 4], the smallest ``dist``, the lowest pair
        index that attains it, the number of pairs with ``dist < margin`` and
        ``sum_p max(0, margin - dist_p)``, a reward's self-collision penalty.
        ``dist`` and ``summary`` do not depend on where the env stands, and
        ``summary`` has the same bits from call to call.  ``out``,
        ``out_witness`` and ``out_summary`` are checked and, for a requested
        part, written and returned as given; without them the tensors are owned
        by the sim, overwritten by the next call with as many pairs and
        replaced by a call with another count."""
        def checked(t, shape, what):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != "cuda" or \
                    t.device.index != (self.device.index or 0):
                raise ValueError(f"{what} must be a float32 tensor on {self.device}")
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{what} must be contiguous with shape {shape}, got {tuple(t.shape)}")
            return t

        def own(key, shape):
            buf = getattr(self, "_prox_out", None)
            if buf is None:
                buf = self._prox_out = {}
            if key not in buf or tuple(buf[key].shape) != shape:   # one tensor per output: a new P replaces it
                buf[key] = torch.zeros(*shape, dtype=torch.float32, device=self.device)
            return buf[key]

        margin = float(margin)
        if not math.isfinite(margin):
            raise ValueError(f"margin must be finite, got {margin}")
        capsules = list(capsules)
        Cn = len(capsules)
        if not 1 <= Cn <= abi.TG_PROX_MAX_CAPSULES:
            raise ValueError(f"proximity takes 1..{abi.TG_PROX_MAX_CAPSULES} capsules, got {Cn}")
        if not all(isinstance(c, abi.tg_capsule) for c in capsules):
            raise ValueError("capsules must be tg_capsule (Sim.capsule, Sim.limb_capsule)")
        flat = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
        P = int(flat.shape[0])
        if not 1 <= P <= abi.TG_PROX_MAX_PAIRS:
            raise ValueError(f"proximity takes 1..{abi.TG_PROX_MAX_PAIRS} pairs, got {P}")
        if flat.min() < 0 or flat.max() >= Cn or bool((flat[:, 0] == flat[:, 1]).any()):
            raise ValueError(f"a pair must name two different capsules in [0, {Cn})")
        if not (dist or witness or summary):
            raise ValueError("proximity needs one of dist, witness and summary")
        N = self.num_envs
        shapes = {"out": (N, P), "out_witness": (N, P, 6), "out_summary": (N, 4)}
        given = {"out": out, "out_witness": out_witness, "out_summary": out_summary}
        for key, t in given.items():
            if t is not None:
                checked(t, shapes[key], key)
        dt, wt, st = ((given[key] if given[key] is not None else own(key, shapes[key])) if asked else None
                      for key, asked in (("out", dist), ("out_witness", witness), ("out_summary", summary)))
        pp = abi.tg_proximity_params()
        pp.margin = margin
        arr = (abi.tg_capsule * Cn)(*capsules)
        idx = (C.c_int32 * (2 * P))(*[int(v) for v in flat.reshape(-1)])
        check(lib().tg_proximity(self._h, arr, Cn, idx, P, C.byref(pp), _ptr(dt), _ptr(wt), _ptr(st)), "proximity")
        return Proximity(dt, wt, st)

    @property
    def contact_link_indices(self) -> list:
        return contact_link_indices(self.model)

    def sync(self):
        check(lib().tg_sync(self._h), "sync")

    def set_kernel_timing(self, period: int):
        """Bracket every ``period``-th articulation step kernel launch with HIP
        events on the sim stream (``True``/1: every launch, 0/``False``: off);
        a negative period -W brackets windows of W consecutive step-kernel
        launches with one event pair (a window another launch of the library
        falls into is dropped)."""
        check(lib().tg_set_kernel_timing(self._h, int(period)), "set_kernel_timing")

    def read_kernel_timing(self):
        """(total kernel ms, launches) since the last read; waits for the recorded launches."""
        ms, n = C.c_double(), C.c_int64()
        check(lib().tg_read_kernel_timing(self._h, C.byref(ms), C.byref(n)), "read_kernel_timing")
        return ms.value, n.value

    def close(self):
        if getattr(self, "_h", None):
            lib().tg_sim_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- helpers
    def _dev(self, t: torch.Tensor) -> torch.Tensor:
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"expected a contiguous float32 tensor on {self.device}, got {t.dtype} on {t.device}")
        return t

    def _ids(self, ids: torch.Tensor) -> torch.Tensor:
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        return ids

    def props_view(self, field: int) -> torch.Tensor:
        """[N,D] live view of one per-env DOF property field (tgsim.h TG_PROP_*)."""
        return self.dof_props[field]
