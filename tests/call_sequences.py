"""Harness of the call-sequence tests (tests/test_gpu_call_sequences.py).

The host side of the library (csrc/tgsim_api.cpp) decides per simulate which
launches it can skip, from a handful of flags every entry point edits
(DESIGN.md §4.2).  The tests run one scripted sequence of calls on a sim
created with the default environment and on a control created under the
library's cache-free switches, and require bit-identical states after every
simulate.  This module holds what the rows share: creation under switches,
the launch-statistics read-out, the raw ``Sim`` set-ups with their seeded
inputs, snapshots and their comparison."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from thormang_isaacgym_amd import abi
from thormang_isaacgym_amd._lib import check, lib

DEV = "cuda:0"
#: every switch tg_sim_create or a task step reads from the environment
SWITCHES = ("TG_ALWAYS_COMPOSE", "TG_NO_SHARED_CACHE", "TG_SEAT_RECOMPOSE", "TG_WALK_UNFUSED", "TG_POST_UNFUSED",
            "TG_PRE_IN_COMPOSE", "TG_PAPER_TWO_LAUNCH", "TG_PAPER_FINISH", "TG_PAPER_RB_LAUNCH", "TG_PAPER_UNFUSED")
#: the cache-free control of the raw-Sim rows
CONTROL = {"TG_ALWAYS_COMPOSE": "1", "TG_NO_SHARED_CACHE": "1"}
#: tg_debug_launch_stats' counters, in order
STATS = ("full", "list", "skipped", "rb_launch", "rb_in_compose", "declined")


def create_under(monkeypatch, switches, factory):
    """``factory()`` with exactly ``switches`` set in the environment (the
    library reads them when the sim is created); they are deleted again
    right after, so nothing later in the test or the session sees them."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    try:
        return factory()
    finally:
        for k in switches:
            monkeypatch.delenv(k, raising=False)


def launch_stats(sim) -> dict:
    out = (C.c_int64 * len(STATS))()
    check(lib().tg_debug_launch_stats(sim.handle, out), "tg_debug_launch_stats")
    return dict(zip(STATS, (int(x) for x in out)))


def since(sim, before: dict) -> dict:
    """the counters' growth since the read-out ``before``"""
    now = launch_stats(sim)
    return {k: now[k] - before[k] for k in STATS}


# ---------------------------------------------------------------- raw sims
def walk_sim(n: int, substeps: int | None = None, seed: int = 3):
    """A raw ``Sim`` of the thormang model set up as the walk task does (PD
    drives on every joint, the cfg's sim parameters), standing on the ground
    with seeded per-env joint offsets so that no two envs share a state.
    Every env has the same properties and masses: the batch is uniform and
    the shared composite cache is in use after the first simulate."""
    from thormang_isaacgym_amd.cfg import load_task_cfg
    from thormang_isaacgym_amd.sim import Sim, load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_asset_options, walk_dof_props
    cfg = load_task_cfg("ThormangWalk", num_envs=n)
    m = load_model("thormang")
    sim_cfg = dict(cfg["sim"])
    if substeps is not None:
        sim_cfg["substeps"] = substeps
    sp = abi.sim_params_from_cfg(sim_cfg, walk_asset_options(cfg), n, float(cfg["env"].get("envSpacing", 1.0)),
                                 warn=False, default_contact_offset=0.016)
    s = Sim(m, sp, n, DEV)
    props, _, default = walk_dof_props(m, cfg, n)
    s.dof_props.copy_(torch.from_numpy(props))
    s.env_dirty.fill_(1)
    s.refresh()
    s.root_state[:, 2] = float(cfg["env"].get("spawnHeight", 0.79))
    rs = np.random.default_rng(seed)
    q = default[None, :] + rs.normal(0.0, 0.03, (n, m.num_dof)).astype(np.float32)
    s.dof_state.view(n, m.num_dof, 2)[..., 0] = torch.from_numpy(q).to(DEV)
    return s


@functools.lru_cache(maxsize=None)
def walk_targets(n: int, steps: int, seed: int = 17):
    """``steps`` position-target tensors [n, 33] around the walk's default
    pose, drawn once per (n, steps, seed) and shared by every sim and test
    that asks for them (read-only)."""
    from thormang_isaacgym_amd.cfg import load_task_cfg
    from thormang_isaacgym_amd.sim import load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_dof_props
    m = load_model("thormang")
    _, _, default = walk_dof_props(m, load_task_cfg("ThormangWalk", num_envs=n), n)
    rs = np.random.default_rng(seed)
    return tuple(torch.from_numpy(default[None, :] + rs.uniform(-0.15, 0.15, (n, m.num_dof)).astype(np.float32))
                 .to(DEV).contiguous() for _ in range(steps))


def gogoro_sim(n: int, seed: int = 5):
    """A raw ``Sim`` of the gogoro model with the task's initial DOF
    properties (the joints_pos lock windows, wheel and steering drives), the
    three seat locks at a 1e-4 window from 0, the rider in the reset pose and
    seeded rear-wheel speeds and steering targets per env.  Returns the sim
    and the model's DOF name -> index map."""
    from thormang_isaacgym_amd.cfg import load_task_cfg
    from thormang_isaacgym_amd.sim import Sim, load_model
    from thormang_isaacgym_amd.tasks.gogoro_cfg import ASSET_OPTIONS, SEAT_DOFS, initial_dof_props, thormang_pose
    cfg = load_task_cfg("Gogoro", num_envs=n)
    m = load_model("gogoro")
    dni = m.dof_name_to_id()
    sp = abi.sim_params_from_cfg(cfg["sim"], dict(ASSET_OPTIONS), n, 1.0, warn=False)
    s = Sim(m, sp, n, DEV)
    props = initial_dof_props(m, cfg, n)
    for name in SEAT_DOFS:
        props[abi.TG_PROP_LOWER, :, dni[name]] = 0.0
        props[abi.TG_PROP_UPPER, :, dni[name]] = 1e-4
    s.dof_props.copy_(torch.from_numpy(props))
    s.env_dirty.fill_(1)
    s.refresh()
    s.root_state[:, 2] = 0.03
    pose = thormang_pose(cfg, dni)
    for name in SEAT_DOFS:
        pose[dni[name]] = 0.5e-4
    s.dof_state.view(n, m.num_dof, 2)[..., 0] = torch.from_numpy(pose).to(DEV)[None, :]
    rs = np.random.default_rng(seed)
    vt = np.zeros((n, m.num_dof), np.float32)
    pt = np.zeros((n, m.num_dof), np.float32)
    vt[:, dni["rear_wheel_joint"]] = rs.uniform(2.0, 8.0, n)
    pt[:, dni["steering_joint"]] = rs.uniform(-0.3, 0.3, n)
    s.set_dof_velocity_targets(torch.from_numpy(vt).to(DEV))
    s.set_dof_position_targets(torch.from_numpy(pt).to(DEV))
    return s, dni


def mass_rows(sim, ids, scale: float) -> torch.Tensor:
    """[N, L] mass scales: the sim's current ones with the rows ``ids`` set to ``scale`` on every link"""
    ms = sim.body_mass_scale.clone()
    ms[torch.as_tensor(ids, dtype=torch.long, device=ms.device)] = scale
    return ms.contiguous()


def ids32(ids) -> torch.Tensor:
    return torch.as_tensor(list(ids), dtype=torch.int32, device=DEV)


def composite_recompose(sim):
    """tg_composite(recompose=1): every env re-composed from scratch (the
    copy of the cache goes to a scratch buffer)"""
    out = torch.empty(sim.num_envs * 4096, device=DEV)
    check(lib().tg_composite(sim.handle, C.c_void_p(out.data_ptr()), 1), "tg_composite")
    return out


def rebind(sim, names=("dof_props", "env_dirty", "root_state")):
    """tg_bind_state to fresh tensors for ``names`` (the library copies the
    live contents over and switches to them); the ``Sim``'s views follow.  The
    new tensors start out as NaN / 0xFF so that a missed copy shows."""
    v = abi.tg_state_view()
    new = {}
    for k in names:
        old = getattr(sim, k)
        new[k] = torch.full_like(old, 255 if old.dtype == torch.uint8 else float("nan"))
        setattr(v, k, new[k].data_ptr())
    check(lib().tg_bind_state(sim.handle, C.byref(v)), "tg_bind_state")
    for k, t in new.items():
        setattr(sim, k, t)


def contact_tensor_off(sim):
    check(lib().tg_set_net_contact_force_tensor(sim.handle, None), "tg_set_net_contact_force_tensor(NULL)")
    sim.net_contact_force = None


def dof_force_tensor_off(sim):
    check(lib().tg_set_dof_force_tensor(sim.handle, None), "tg_set_dof_force_tensor(NULL)")
    sim.dof_force = None


# ---------------------------------------------------------------- snapshots
def snap_sim(sim) -> dict:
    d = {"root_state": sim.root_state.clone(), "dof_state": sim.dof_state.clone()}
    for k in ("net_contact_force", "dof_force"):
        t = getattr(sim, k, None)
        if t is not None:
            d[k] = t.clone()
    return d


def snap_env(env) -> dict:
    d = snap_sim(env.sim)
    for k in ("obs_buf", "rew_buf", "reset_buf", "progress_buf"):
        d[k] = getattr(env, k).clone()
    return d


def env_rows(snap: dict, n: int) -> torch.Tensor:
    """[n, *] root and DOF state of a snapshot, one row per env"""
    return torch.cat([snap["root_state"].view(n, -1), snap["dof_state"].view(n, -1)], 1)


def changed_envs(a: dict, b: dict, n: int) -> set:
    """the envs whose root or DOF state differs in any bit between two snapshots"""
    return set((env_rows(a, n) != env_rows(b, n)).any(1).nonzero().flatten().tolist())


def assert_same(a: list, b: list, what: str, keys=None, steps=None):
    """Two traces (one snapshot per simulate) agree bit for bit in every
    tensor both hold (``keys``: only these; ``steps``: only these steps); the
    message names the first step, tensor and env rows that differ."""
    assert len(a) == len(b), (what, len(a), len(b))
    for t, (x, y) in enumerate(zip(a, b)):
        if steps is not None and t not in steps:
            continue
        for k in (keys or sorted(set(x) & set(y))):
            if not torch.equal(x[k], y[k]):
                n = x["root_state"].shape[0]
                rows = (x[k].reshape(n, -1) != y[k].reshape(n, -1)).any(1).nonzero().flatten().tolist()
                diff = float((x[k].double() - y[k].double()).abs().max())
                raise AssertionError(f"{what}: step {t}, {k}: envs {rows} differ (max |a - b| = {diff:.3g})")
        assert all(torch.isfinite(x[k]).all() for k in ("root_state", "dof_state")), (what, t, "non-finite state")


def transplant(src, dst):
    """Copy everything a simulate reads from sim ``src`` into the freshly
    created ``dst``: root and DOF state, the three target tensors, the DOF
    properties, mass scales and friction."""
    for k in ("root_state", "dof_state", "dof_pos_target", "dof_vel_target", "dof_actuation", "dof_props"):
        getattr(dst, k).copy_(getattr(src, k))
    dst.env_dirty.fill_(1)
    dst.refresh()
    dst.set_body_mass_scale_indexed(src.body_mass_scale.clone().contiguous(), dst.all_ids)
    dst.set_shape_friction_indexed(src.shape_friction.clone().contiguous(), dst.all_ids)
