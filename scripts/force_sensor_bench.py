"""Developer micro-benchmark of the force sensor tensor
(tg_set_force_sensor_tensor): the step kernel's own time on 4096 envs of the
Thormang model set up as the walk task does, standing on both feet, with no
export tensor (NoPost), with the net contact force tensor (NoPostCF), with the
contact and the DOF force tensor (NoPostDF) and with the sensor tensor on
(NoPostFS): two sensors at the soles' centres in local space, alone and beside
the other two, and eight sensors.

Every variant starts every block from the same state and simulates 200 times
with HIP events around each step kernel launch (Sim.set_kernel_timing);
seven alternating blocks, median (min-max) per launch.  The states stay
bit-identical between the variants, which the script checks, so every variant
times the same work plus its own export.  No GPU, no figure: the script fails
without one.

    python scripts/force_sensor_bench.py
"""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd._lib import check, lib  # noqa: E402
from thormang_isaacgym_amd.cfg import load_task_cfg  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402
from thormang_isaacgym_amd.tasks.thormang_walk import (walk_asset_options, walk_dof_props, walk_feet_indices,  # noqa: E402
                                                      walk_sole_centre)

N, BLOCKS, CALLS = 4096, 7, 200
DEV = "cuda:0"


def main():
    assert torch.cuda.is_available(), "force_sensor_bench needs the MI355X"
    cfg = load_task_cfg("ThormangWalk", num_envs=N)
    m = load_model("thormang")
    sp = abi.sim_params_from_cfg(dict(cfg["sim"]), walk_asset_options(cfg), N, float(cfg["env"].get("envSpacing", 1.0)),
                                 warn=False, default_contact_offset=0.016)
    s = Sim(m, sp, N, DEV)
    props, _, default = walk_dof_props(m, cfg, N)
    s.dof_props.copy_(torch.from_numpy(props))
    s.env_dirty.fill_(1)
    s.refresh()
    s.root_state[:, 2] = float(cfg["env"].get("spawnHeight", 0.79))
    rs = np.random.default_rng(3)
    q = default[None, :] + rs.normal(0.0, 0.03, (N, m.num_dof)).astype(np.float32)
    s.dof_state.view(N, m.num_dof, 2)[..., 0] = torch.from_numpy(q).to(DEV)
    s.set_dof_position_targets(torch.from_numpy(np.repeat(default[None, :], N, 0)).to(DEV).contiguous())
    for _ in range(30):   # down on both feet
        s.simulate()
    root0, dof0 = s.root_state.clone(), s.dof_state.clone()
    feet = walk_feet_indices(m)
    two = [s.contact_frame(l, walk_sole_centre(m, l)) for l in feet]
    eight = [s.contact_frame(feet[k % 2], (0.02 * k, 0.0, -0.0275)) for k in range(8)]
    L = lib()

    def setup(cf, df, sensors):
        def f():
            check(L.tg_set_net_contact_force_tensor(s.handle, None), "off")
            check(L.tg_set_dof_force_tensor(s.handle, None), "off")
            s.acquire_force_sensor_tensor([])
            s.net_contact_force = s.dof_force = None
            out = []
            if cf:
                out.append(s.acquire_net_contact_force_tensor())
            if df:
                out.append(s.acquire_dof_force_tensor())
            if sensors:
                out.append(s.acquire_force_sensor_tensor(sensors, space="local"))
            return out
        return f

    variants = [("no export tensor (NoPost)", setup(False, False, None)),
                ("contact force tensor (NoPostCF)", setup(True, False, None)),
                ("contact + DOF force tensors (NoPostDF)", setup(True, True, None)),
                ("sensor tensor, 2 sensors (NoPostFS)", setup(False, False, two)),
                ("sensor tensor, 2 sensors + contact + DOF force (NoPostFS)", setup(True, True, two)),
                ("sensor tensor, 8 sensors (NoPostFS)", setup(False, False, eight))]
    times = {nm: [] for nm, _ in variants}
    end, load = {}, {}
    for b in range(BLOCKS + 1):   # (block 0 warms every variant up)
        for nm, prep in variants:
            keep = prep()
            s.root_state.copy_(root0)
            s.dof_state.copy_(dof0)
            s.set_kernel_timing(1)
            for _ in range(CALLS):
                s.simulate()
            ms, n = s.read_kernel_timing()
            s.set_kernel_timing(0)
            assert n == CALLS, (nm, n)
            if b:
                times[nm].append(ms / n * 1e3)
            end[nm] = (s.root_state.clone(), s.dof_state.clone())
            if "sensor" in nm:
                load[nm] = float(keep[-1][:, :, 2].sum(1).mean())
    ref = end[variants[0][0]]
    same = all(torch.equal(e[0], ref[0]) and torch.equal(e[1], ref[1]) for e in end.values())
    print(f"thormang (walk set-up): N = {N}, substeps = {int(sp.substeps)}, {CALLS} simulates per block, {BLOCKS} blocks; "
          f"end states bit-identical across the variants: {same}; mean f_z over the feet "
          f"{load[variants[3][0]]:.1f} N")
    base = statistics.median(times[variants[2][0]])
    for nm, _ in variants:
        t = times[nm]
        print(f"  {nm:60s} {statistics.median(t):8.2f} us ({min(t):.2f}-{max(t):.2f})   "
              f"{statistics.median(t) - base:+6.2f} us against NoPostDF")
    print(f"  bytes written per launch: sensors 2 x 24 B/env = {N * 48 / 1e6:.2f} MB, contact tensor "
          f"{N * s.L * 12 / 1e6:.2f} MB (2 of {s.L} links written), DOF force tensor {N * s.D * 4 / 1e6:.2f} MB")
    assert same


if __name__ == "__main__":
    main()
