"""Developer micro-benchmark of the contact-consistent inverse dynamics
(tg_contact_inverse_dynamics) at 4096 envs on Thormang, K = 2 (the feet) and
K = 4 (feet and arm end links), with and without the wrench and efforts
outputs, beside tg_inverse_dynamics and beside what a user had before it, the
tensor route: refresh the Jacobian tensor, inverse_dynamics, a batched 6 x 6
solve in torch and two einsums.  The tensor route is timed in its cheapest
form, with the contact points at the links' centres of mass, so that the point
Jacobians are rows of the Jacobian tensor and no lever arm has to be formed;
for those contacts both sides compute the same torques (the largest difference
is printed).

HIP events around blocks of back-to-back calls (2000 of the fused calls, 100 of
the tensor route, so that every window is tens of milliseconds), seven
alternating blocks, median (min-max) per call; the host time to enqueue a call
is printed too, so a figure that is the enqueue rate and not the device's
duration can be told apart.  No GPU, no figure: the script fails without one.

    python scripts/contact_id_bench.py
"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd._lib import check, lib  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402

N, BLOCKS = 4096, 7
GRAVITY = (0.0, 0.0, -9.81)
MOMENT_ARM = 0.1
LINKS = ["l_leg_foot_link", "r_leg_foot_link", "l_arm_end_link", "r_arm_end_link"]


def main():
    assert torch.cuda.is_available(), "contact_id_bench needs the MI355X"
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
    eff = torch.zeros(N, D, device=dev)
    tau = torch.zeros(N, 6 + D, device=dev)
    b = torch.zeros(N, 6 + D, device=dev)
    tau_t = torch.zeros(N, 6 + D, device=dev)
    J = s.acquire_jacobian_tensor()
    li = np.asarray(abi.model_arrays(m)["link_inertia"], np.float32)
    names = [l.name for l in m.links]
    links = [names.index(x) for x in LINKS]
    # the contact points at the links' coms: Jp_k = J[:, l_k]
    frames = {K: (abi.tg_contact_frame * K)(*[s.contact_frame(l, li[l, 1:4]) for l in links[:K]]) for K in (2, 4)}
    wrench = {K: torch.zeros(N, K, 6, device=dev) for K in (2, 4)}
    share = {K: torch.rand(N, K, device=dev, generator=g) * 0.9 + 0.1 for K in (2, 4)}
    dm = torch.tensor([1.0, 1.0, 1.0] + [MOMENT_ARM ** 2] * 3, device=dev)
    idx = {K: torch.tensor(links[:K], device=dev) for K in (2, 4)}
    L = lib()

    def cid(K, with_wrench, with_efforts, with_share=False):
        def f():
            check(L.tg_contact_inverse_dynamics(s.handle, frames[K], K, share[K].data_ptr() if with_share else None,
                                                MOMENT_ARM, 3, None, tau.data_ptr(),
                                                wrench[K].data_ptr() if with_wrench else None,
                                                eff.data_ptr() if with_efforts else None, None, 0, 0), "bench")
        return f

    def plain():
        s.inverse_dynamics(out=b)

    def tensor_route(K):
        def f():
            s.refresh_jacobian_tensors()
            s.inverse_dynamics(out=b)
            Jp = J[:, idx[K]]                                           # [N, K, 6, 6 + D]
            G = Jp[..., :6].transpose(2, 3)                             # [N, K, 6, 6]
            A = torch.einsum("ekij,j,eklj->eil", G, dm, G)
            y = torch.linalg.solve(A, b[:, :6])
            lam = dm * torch.einsum("ekji,ej->eki", G, y)
            tau_t.copy_(b - torch.einsum("ekic,eki->ec", Jp, lam))
        return f

    variants = [("tg_contact_inverse_dynamics K = 2 (tau)", cid(2, False, False), 2000),
                ("tg_contact_inverse_dynamics K = 2 (tau + wrench)", cid(2, True, False), 2000),
                ("tg_contact_inverse_dynamics K = 2 (tau + wrench + efforts)", cid(2, True, True), 2000),
                ("tg_contact_inverse_dynamics K = 2 (all + share tensor)", cid(2, True, True, True), 2000),
                ("tg_contact_inverse_dynamics K = 4 (tau)", cid(4, False, False), 2000),
                ("tg_contact_inverse_dynamics K = 4 (tau + wrench)", cid(4, True, False), 2000),
                ("tg_contact_inverse_dynamics K = 4 (tau + wrench + efforts)", cid(4, True, True), 2000),
                ("tg_contact_inverse_dynamics K = 4 (all + share tensor)", cid(4, True, True, True), 2000),
                ("tg_inverse_dynamics (gravity + velocity)", plain, 2000),
                ("tensor route K = 2 (refresh J + ID + torch solve)", tensor_route(2), 100),
                ("tensor route K = 4 (refresh J + ID + torch solve)", tensor_route(4), 100)]
    for _, f, _n in variants:                                 # warm every shape
        for _ in range(3):
            f()
    for K in (2, 4):
        cid(K, True, False)()
        tensor_route(K)()
        torch.cuda.synchronize()
        scale = float(tau[:, 6:].abs().max())
        print(f"thormang: N = {N}, D = {D}, L = {s.L}, K = {K}; max |tau(tensor route) - tau(kernel)| / max |tau| = "
              f"{float((tau_t[:, 6:] - tau[:, 6:]).abs().max()) / scale:.2e} (max |tau| = {scale:.1f})")
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
        print(f"  {nm:60s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
              f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    print(f"  bytes written per call: tau {tau.numel() * 4 / 1e6:.2f} MB ({(6 + D) * 4} B/env), wrench K = 4 "
          f"{wrench[4].numel() * 4 / 1e6:.2f} MB; the Jacobian tensor {J.numel() * 4 / 1e6:.1f} MB "
          f"({J.numel() * 4 / N / 1024:.1f} KB/env)")


if __name__ == "__main__":
    main()
