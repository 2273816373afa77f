"""Developer micro-benchmark of the operational-space control (tg_osc) at 4096
envs on Thormang with the two 7-DOF arm chains, against the composition it
replaces (tasks/franka_cube_stack.py:440-441, 602-628): refresh the Jacobian
and the mass-matrix tensors, slice one link's 6 x 7 block and the chain's 7 x 7
block, two torch.inverse, the matmuls of _compute_osc_torques with its
null-space term, the clamp to the effort limits.  The pose error is handed to
the torch path ready-made, so it is charged less than the reference pays, and
it adds the same lambda^2 I to the task-space matrix, so both sides compute
the same torques (the largest difference is printed: the arm end links have
their centre of mass at the origin, where the Jacobian tensor's point and the
kernel's agree).

HIP events around blocks of back-to-back calls (2000 of the fused call, 200 of
each slower variant, so that every window is tens of milliseconds), seven
alternating blocks, median (min-max) per call; the host time to enqueue a call
is printed too, so a figure that is the enqueue rate and not the device's
duration can be told apart.  No GPU, no figure: the script fails without one.

    python scripts/osc_bench.py
"""
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402

N, BLOCKS = 4096, 7
KP, KP_NULL, DAMPING = 150.0, 10.0, 1e-2
KD, KD_NULL = 2 * math.sqrt(KP), 2 * math.sqrt(KP_NULL)


def main():
    assert torch.cuda.is_available(), "osc_bench needs the MI355X"
    m = load_model("thormang")
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0, 0, -9.81]}, {}, N)
    s = Sim(m, sp, N, "cuda:0")
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :3] = torch.randn(N, 3, device=dev, generator=g)
    q = torch.randn(N, 4, device=dev, generator=g)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 2 - 1
    s.dof_state[:, 1] = torch.randn(N * s.D, device=dev, generator=g)
    props = torch.from_numpy(abi.default_dof_props(m, N))
    props[abi.TG_PROP_ARMATURE] = 0.01
    s.dof_props.copy_(props)
    s.refresh()
    chains = [s.ik_chain("l_arm_end_link", num_dofs=7), s.ik_chain("r_arm_end_link", num_dofs=7)]
    K = len(chains)
    gp = (s.root_state[:, None, :3] + torch.rand(N, K, 3, device=dev, generator=g) - 0.5).contiguous()
    gq = torch.randn(N, K, 4, device=dev, generator=g)
    state = s.dof_state.view(N, s.D, 2)
    rest = (state[:, :, 0] + torch.rand(N, s.D, device=dev, generator=g) - 0.5).contiguous()
    eff = torch.zeros(N, s.D, device=dev)
    eff_b = torch.zeros(N, s.D, device=dev)
    kw = dict(q_rest=rest, kp=KP, kp_null=KP_NULL, damping=DAMPING)
    tau, err = s.solve_osc(chains, gp, gq, efforts=eff, return_error=True, **kw)
    J, H = s.acquire_jacobian_tensor(), s.acquire_mass_matrix_tensor()
    dofs = [torch.tensor([int(c.dofs[i]) for i in range(c.num_dofs)], device=dev) for c in chains]
    cols = [d + 6 for d in dofs]
    lam = torch.eye(6, device=dev) * DAMPING ** 2
    eye7 = torch.eye(7, device=dev).unsqueeze(0)
    dpose = err.clone()                                        # [N, K, 6]
    limit = s.dof_props[abi.TG_PROP_EFFORT]
    tau_b = torch.zeros(N, K, 7, device=dev)

    def fused():
        s.solve_osc(chains, gp, gq, efforts=eff, **kw)

    def fused_no_null():
        s.solve_osc(chains, gp, gq, efforts=eff, kp=KP, damping=DAMPING)

    def refresh_only():
        s.refresh_jacobian_tensors()
        s.refresh_mass_matrix_tensors()

    def composition():
        s.refresh_jacobian_tensors()
        s.refresh_mass_matrix_tensors()
        for k, c in enumerate(chains):
            qk, qdk = state[:, dofs[k], 0], state[:, dofs[k], 1]
            j_eef = J[:, c.link, :, cols[k]]
            mm = H[:, cols[k]][:, :, cols[k]]
            mm_inv = torch.inverse(mm)
            j_t = torch.transpose(j_eef, 1, 2)
            m_eef = torch.inverse(j_eef @ mm_inv @ j_t + lam)
            eef_vel = (j_eef @ qdk.unsqueeze(-1)).squeeze(-1)
            u = j_t @ m_eef @ (KP * dpose[:, k] - KD * eef_vel).unsqueeze(-1)
            j_eef_inv = m_eef @ j_eef @ mm_inv
            u_null = KD_NULL * -qdk + KP_NULL * ((rest[:, dofs[k]] - qk + math.pi) % (2 * math.pi) - math.pi)
            u_null = mm @ u_null.unsqueeze(-1)
            u += (eye7 - j_t @ j_eef_inv) @ u_null
            tau_b[:, k] = u.squeeze(-1)
            eff_b[:, dofs[k]] = torch.max(torch.min(tau_b[:, k], limit[:, dofs[k]]), -limit[:, dofs[k]])

    variants = [("tg_osc (tau, err, efforts; null space)", fused, 2000), ("tg_osc (no q_rest)", fused_no_null, 2000),
                ("the two refreshes alone", refresh_only, 200), ("refreshes + the reference's torch formula", composition, 200)]
    for _, f, _n in variants:                                 # warm every shape
        for _ in range(3):
            f()
    fused()
    torch.cuda.synchronize()
    scale = float(tau.abs().max())
    d_tau = float((tau_b - tau[:, :, :7]).abs().max()) / scale
    d_eff = max(float((eff_b[:, d] - eff[:, d]).abs().max()) for d in dofs) / scale
    print(f"thormang: {K} arm chains of 7 DOFs, N = {N}; max |tau(torch) - tau(kernel)| / max |tau| = {d_tau:.2e}, "
          f"efforts {d_eff:.2e} (max |tau| = {scale:.1f})")
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
        print(f"  {nm:44s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
              f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    out_b = (tau.numel() + err.numel()) * 4 + N * sum(c.num_dofs for c in chains) * 4
    print(f"  bytes written per call: tg_osc {out_b / 1e6:.2f} MB ({out_b / N:.0f} B/env); the two tensors "
          f"{(J.numel() + H.numel()) * 4 / 1e6:.1f} MB ({(J.numel() + H.numel()) * 4 / N / 1024:.1f} KB/env)")


if __name__ == "__main__":
    main()
