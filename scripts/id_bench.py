"""Developer micro-benchmark of the inverse dynamics (tg_inverse_dynamics) at
4096 envs on Thormang, against what a user had before it: refresh the Jacobian
tensor and sum -s_l m_l Jv_l^T g over the links in torch -- the gravity term
only, the Coriolis term cannot be had that way -- and against
refresh_mass_matrix_tensors, the kernel it shares its kinematics and its
inward pass with.  Both sides compute the same gravity torques (the largest
difference is printed).

HIP events around blocks of back-to-back calls (2000 of the fused call, 200 of
each slower variant, so that every window is tens of milliseconds), seven
alternating blocks, median (min-max) per call; the host time to enqueue a call
is printed too, so a figure that is the enqueue rate and not the device's
duration can be told apart.  No GPU, no figure: the script fails without one.

    python scripts/id_bench.py
"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402

N, BLOCKS = 4096, 7
GRAVITY = (0.0, 0.0, -9.81)


def main():
    assert torch.cuda.is_available(), "id_bench needs the MI355X"
    m = load_model("thormang")
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": list(GRAVITY)}, {}, N)
    s = Sim(m, sp, N, "cuda:0")
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :3] = torch.randn(N, 3, device=dev, generator=g)
    q = torch.randn(N, 4, device=dev, generator=g)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.root_state[:, 7:13] = torch.randn(N, 6, device=dev, generator=g)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 2 - 1
    s.dof_state[:, 1] = torch.randn(N * s.D, device=dev, generator=g)
    props = torch.from_numpy(abi.default_dof_props(m, N))
    props[abi.TG_PROP_ARMATURE] = 0.01
    s.dof_props.copy_(props)
    s.refresh()
    D = s.D
    accel = torch.randn(N, 6 + D, device=dev, generator=g)
    eff = torch.zeros(N, D, device=dev)
    arm_dofs = [d for d, nm in enumerate(m.dof_names) if "_arm_" in nm]
    tau = torch.zeros(N, 6 + D, device=dev)
    J = s.acquire_jacobian_tensor()
    s.acquire_mass_matrix_tensor()
    mass = torch.from_numpy(np.asarray(abi.model_arrays(m)["link_inertia"], np.float32)[:, 0].copy()).to(dev)
    mg = -(mass[:, None] * torch.tensor(GRAVITY, device=dev)[None, :])      # [L, 3]: -m_l g
    tau_b = torch.zeros(N, 6 + D, device=dev)

    def both():
        s.inverse_dynamics(out=tau)

    def gravity_only():
        s.inverse_dynamics(velocity=False, out=tau)

    def full():
        s.inverse_dynamics(accel=accel, out=tau)

    def efforts_accumulate():
        s.inverse_dynamics(dofs=arm_dofs, efforts=eff, accumulate=True, out=tau)

    def refresh_jac():
        s.refresh_jacobian_tensors()

    def jac_gravity_sum():
        s.refresh_jacobian_tensors()
        tau_b.copy_(torch.einsum("elkc,lk->ec", J[:, :, :3], mg))

    def refresh_mass():
        s.refresh_mass_matrix_tensors()

    variants = [("tg_inverse_dynamics (gravity + velocity)", both, 2000),
                ("tg_inverse_dynamics (gravity only)", gravity_only, 2000),
                ("tg_inverse_dynamics (both + accel)", full, 2000),
                ("tg_inverse_dynamics (+ efforts, accumulate, arm DOFs)", efforts_accumulate, 2000),
                ("refresh_jacobian_tensors alone", refresh_jac, 200),
                ("refresh_jacobian_tensors + torch gravity sum", jac_gravity_sum, 200),
                ("refresh_mass_matrix_tensors", refresh_mass, 200)]
    for _, f, _n in variants:                                 # warm every shape
        for _ in range(3):
            f()
    gravity_only()
    jac_gravity_sum()
    torch.cuda.synchronize()
    scale = float(tau.abs().max())
    print(f"thormang: N = {N}, D = {D}, L = {s.L}; max |tau_g(torch sum) - tau_g(kernel)| / max |tau_g| = "
          f"{float((tau_b - tau).abs().max()) / scale:.2e} (max |tau_g| = {scale:.1f})")
    times = {nm: [] for nm, _, _ in variants}
    host = {nm: [] for nm, _, _ in variants}
    for _ in range(BLOCKS):
        for nm, f, calls in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            host[nm].append((time.perf_counter() - t0) / calls * 1e6)
            torch.cuda.synchronize()
            times[nm].append(e0.elapsed_time(e1) / calls * 1e3)
    for nm, _, calls in variants:
        t = times[nm]
        print(f"  {nm:54s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
              f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    print(f"  bytes written per call: tg_inverse_dynamics {tau.numel() * 4 / 1e6:.2f} MB ({(6 + D) * 4} B/env); the "
          f"Jacobian tensor {J.numel() * 4 / 1e6:.1f} MB ({J.numel() * 4 / N / 1024:.1f} KB/env)")


if __name__ == "__main__":
    main()
