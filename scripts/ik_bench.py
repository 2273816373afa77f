"""Developer micro-benchmark of the damped-least-squares IK (tg_ik_dls) at 4096
envs against (a) tg_jacobians alone and (b) the torch path the reference task
uses on the Jacobian tensor (tasks/gogoro/gogoro.py:396-427: refresh, gather
one block per chain, transpose, bmm, torch.inverse, bmm, add to the targets;
the pose error is handed to it ready-made, so (b) is charged less than the
reference pays).  HIP events around blocks of 100 back-to-back calls, five
alternating blocks, median (min-max) per call; the host time to enqueue a
block is printed too, so a figure that is the enqueue rate and not the
kernel's duration can be told apart.

    python scripts/ik_bench.py [thormang|gogoro ...]
"""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd._lib import lib  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402

N, CALLS, BLOCKS = 4096, 100, 5


def chains_for(name, s):
    if name == "thormang":
        return [s.ik_chain("l_arm_end_link"), s.ik_chain("r_arm_end_link"), s.ik_chain("l_leg_foot_link"),
                s.ik_chain("r_leg_foot_link", offset=(0.05, -0.02, -0.03))]
    return [s.ik_chain("l_arm_end_link", num_dofs=7), s.ik_chain("r_arm_end_link", num_dofs=7)]


def main():
    for name in sys.argv[1:] or ["thormang", "gogoro"]:
        m = load_model(name)
        sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0, 0, -9.81]}, {}, N)
        s = Sim(m, sp, N, "cuda:0")
        g = torch.Generator(device="cuda:0").manual_seed(1)
        s.root_state[:, :3] = torch.randn(N, 3, device="cuda:0", generator=g)
        q = torch.randn(N, 4, device="cuda:0", generator=g)
        s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
        s.dof_state[:, 0] = torch.rand(N * s.D, device="cuda:0", generator=g) * 2 - 1
        chains = chains_for(name, s)
        K = len(chains)
        gp = s.root_state[:, None, :3] + torch.rand(N, K, 3, device="cuda:0", generator=g) - 0.5
        gp = gp.contiguous()
        gq = torch.randn(N, K, 4, device="cuda:0", generator=g)
        tgt = torch.zeros(N, s.D, device="cuda:0")
        dq, err = s.solve_ik(chains, gp, gq, targets=tgt, return_error=True)
        arr = (abi.tg_ik_chain * K)(*chains)
        L, h = lib(), s.handle
        J = s.acquire_jacobian_tensor()
        s.refresh_jacobian_tensors()
        cols = [torch.tensor([6 + int(c.dofs[i]) for i in range(c.num_dofs)], device="cuda:0") for c in chains]
        dofs = [c - 6 for c in cols]
        eye = torch.eye(6, device="cuda:0") * (0.3 ** 2)
        dpose = err.clone().unsqueeze(-1)                     # [N, K, 6, 1]
        tgt_b = torch.zeros(N, s.D, device="cuda:0")
        q_pos = s.dof_state.view(N, s.D, 2)[:, :, 0]

        def ik_full():
            L.tg_ik_dls(h, arr, K, gp.data_ptr(), gq.data_ptr(), 0.3, dq.data_ptr(), err.data_ptr(), tgt.data_ptr())

        def ik_targets_only():
            L.tg_ik_dls(h, arr, K, gp.data_ptr(), gq.data_ptr(), 0.3, None, None, tgt.data_ptr())

        def jac_only():
            s.refresh_jacobian_tensors()

        def torch_path():
            s.refresh_jacobian_tensors()
            test = q_pos.clone()
            for k, c in enumerate(chains):
                j = J[:, c.link, :, cols[k]]
                jt = torch.transpose(j, 1, 2)
                u = (jt @ torch.inverse(j @ jt + eye) @ dpose[:, k]).squeeze(-1)
                test[:, dofs[k]] += u
            tgt_b.copy_(test)

        variants = [("tg_ik_dls (dq, err, targets)", ik_full), ("tg_ik_dls (targets only)", ik_targets_only),
                    ("tg_jacobians alone", jac_only), ("torch path on the Jacobian tensor", torch_path)]
        for _, f in variants:                                 # warm every shape
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        # the arm end links have their com at the origin, so the torch path and the kernel agree there
        arms = [k for k, c in enumerate(chains) if "arm" in m.links[c.link].name]
        dev = max(float((tgt_b[:, dofs[k]] - tgt[:, dofs[k]]).abs().max()) for k in arms)
        print(f"{name}: {K} chains, N = {N}; max |targets(torch) - targets(kernel)| on the arm DOFs: {dev:.2e}")
        times = {nm: [] for nm, _ in variants}
        host = {nm: [] for nm, _ in variants}
        for _ in range(BLOCKS):
            for nm, f in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(CALLS):
                    f()
                e1.record()
                host[nm].append((time.perf_counter() - t0) / CALLS * 1e6)
                torch.cuda.synchronize()
                times[nm].append(e0.elapsed_time(e1) / CALLS * 1e3)
        for nm, _ in variants:
            t = times[nm]
            print(f"  {nm:36s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
                  f"{statistics.median(host[nm]):.1f} us/call")
        out_b = (dq.numel() + err.numel()) * 4 + N * sum(c.num_dofs for c in chains) * 4
        print(f"  bytes written: IK {out_b / 1e6:.2f} MB ({out_b / N:.0f} B/env), Jacobian {J.numel() * 4 / 1e6:.1f} MB "
              f"({J.numel() * 4 / N / 1024:.1f} KB/env)")
        del s


if __name__ == "__main__":
    main()
