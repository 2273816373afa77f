"""Developer micro-benchmark of the contact force distribution (tg_contact_qp) at
4096 envs on Thormang, both soles (walk_sole_patch), tau + wrench + forces + info:

    tg_contact_qp                 16, 32 and 64 iterations
    tg_contact_inverse_dynamics   the same sim and feet, tau + wrench: the floor
                                  (the same passes without the iterations)
    torch composition             the same ADMM for 64 iterations composed in torch
                                  from Sim.inverse_dynamics (b) and the rigid-body
                                  state tensor (the vertices): the dense
                                  (G^T W G + P) inverted once per env, then some
                                  twenty small launches per iteration

The largest difference between the composition's and the kernel's forces is
printed.  The kernels are called through the C function with their argument
arrays built once; HIP events around blocks of back-to-back calls, seven
alternating blocks, median (min-max) per call.  No GPU, no figure: the script
fails without one.

    python scripts/contact_qp_bench.py [--out profiles/r13/contact_qp_timing.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd._lib import check, lib  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402
from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices, walk_sole_patch  # noqa: E402

N, BLOCKS = 4096, 7
MU, ARM = 0.7, 0.1
D_ = abi.TG_QP_DEFAULTS


def quat_rotate(q, v):
    """q [N, 4] xyzw applied to v [N, 3] (or [3])."""
    qv, w = q[..., :3], q[..., 3:4]
    v = v.expand_as(qv)
    t = 2.0 * torch.cross(qv, v, dim=-1)
    return v + w * t + torch.cross(qv, t, dim=-1)


def skew(r):
    z = torch.zeros_like(r[..., 0])
    return torch.stack([torch.stack([z, -r[..., 2], r[..., 1]], -1), torch.stack([r[..., 2], z, -r[..., 0]], -1),
                        torch.stack([-r[..., 1], r[..., 0], z], -1)], -2)


def torch_qp(b6, rb, com0, links, offs, exts, iters):
    """The header's ADMM composed in torch: forces [N, J, 3] from b6 [N, 6] and the rigid-body states rb [N, L, 13]."""
    n, dev = b6.shape[0], b6.device
    sgn = ((1.0, 1.0), (1.0, -1.0), (-1.0, -1.0), (-1.0, 1.0))
    c_root = rb[:, 0, :3] + quat_rotate(rb[:, 0, 3:7], com0)
    pv = []
    for l, off, (hx, hy) in zip(links, offs, exts):
        for v in range(4):
            local = off + torch.tensor([sgn[v][0] * hx, sgn[v][1] * hy, 0.0], device=dev)
            pv.append(rb[:, l, :3] + quat_rotate(rb[:, l, 3:7], local))
    r = torch.stack(pv, 1) - c_root[:, None]                                   # [N, J, 3]
    J = r.shape[1]
    G = torch.cat([torch.eye(3, device=dev).expand(n, J, 3, 3), skew(r)], dim=2)  # [N, J, 6, 3]
    G = G.permute(0, 2, 1, 3).reshape(n, 6, 3 * J)
    W = torch.diag(torch.tensor([1.0, 1.0, 1.0] + [1.0 / ARM ** 2] * 3, device=dev))
    H = G.transpose(1, 2) @ W @ G + (D_["reg"] + D_["rho"]) * torch.eye(3 * J, device=dev)
    Hinv = torch.linalg.inv(H)
    c = (G.transpose(1, 2) @ (W @ b6[..., None]))[..., 0]
    nz = torch.tensor([0.0, 0.0, 1.0], device=dev)
    z = torch.zeros(n, J, 3, device=dev)
    u = torch.zeros_like(z)
    for _ in range(iters):
        x = (Hinv @ (c + D_["rho"] * (z - u).reshape(n, -1))[..., None])[..., 0].reshape(n, J, 3)
        xh = D_["relax"] * x + (1.0 - D_["relax"]) * z
        w = xh + u
        wn = w[..., 2]
        t = w - wn[..., None] * nz
        tn = t.norm(dim=-1)
        inside = (wn >= 0) & (tn <= MU * wn)
        polar = ~inside & (MU * tn <= -wn)
        a = (MU * tn + wn) / (1 + MU * MU)
        edge = a[..., None] * (nz + (MU / tn.clamp(min=1e-30))[..., None] * t)
        z = torch.where(inside[..., None], w, torch.where(polar[..., None], torch.zeros_like(w), edge))
        u = u + xh - z
    return z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r13", "contact_qp_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "contact_qp_bench needs the MI355X"
    dev = "cuda:0"
    m = load_model("thormang")
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0.0, 0.0, -9.81]}, {}, N)
    s = Sim(m, sp, N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :2] = torch.rand(N, 2, device=dev, generator=g) * 90.0
    s.root_state[:, 2] = 0.79
    q = torch.randn(N, 4, device=dev, generator=g) * 0.03
    q[:, 3] = 1.0
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 0.2 - 0.1
    s.dof_state[:, 1] = torch.randn(N * s.D, device=dev, generator=g) * 0.3
    s.refresh()
    accel = torch.randn(N, 6 + s.D, device=dev, generator=g)
    links = walk_feet_indices(m)
    patches = [walk_sole_patch(m, l) for l in links]
    K = len(links)
    frames = (abi.tg_contact_frame * K)(*[s.contact_frame(l, p[0]) for l, p in zip(links, patches)])
    hxy = (C.c_float * (2 * K))(*[v for p in patches for v in p[1]])
    tau, wrench = torch.zeros(N, 6 + s.D, device=dev), torch.zeros(N, K, 6, device=dev)
    forces, info = torch.zeros(N, K, 4, 3, device=dev), torch.zeros(N, 4, device=dev)
    b = torch.zeros(N, 6 + s.D, device=dev)
    rb = s.acquire_rigid_body_state_tensor().view(N, s.L, 13)
    com0 = torch.tensor(np.asarray(abi.model_arrays(m)["link_inertia"], np.float32)[0, 1:4], device=dev)
    offs = [torch.tensor(p[0], device=dev) for p in patches]
    res = {}

    def qp(iters):
        def f():
            check(lib().tg_contact_qp(s.handle, frames, K, hxy, None, None, MU, None, ARM, D_["reg"], D_["rho"],
                                      D_["relax"], iters, 3, accel.data_ptr(), tau.data_ptr(), wrench.data_ptr(),
                                      forces.data_ptr(), info.data_ptr(), None, None, 0, 0), "contact_qp")
        return f

    def cid():
        check(lib().tg_contact_inverse_dynamics(s.handle, frames, K, None, ARM, 3, accel.data_ptr(), tau.data_ptr(),
                                                wrench.data_ptr(), None, None, 0, 0), "contact_inverse_dynamics")

    def compose():
        s.inverse_dynamics(accel=accel, out=b)
        s.refresh_rigid_body_state_tensor()
        res["z"] = torch_qp(b[:, :6], rb, com0, links, offs, [p[1] for p in patches], D_["iters"])

    variants = [(f"tg_contact_qp, {it} iterations", qp(it), 2000) for it in (16, 32, 64)] + \
               [("tg_contact_inverse_dynamics (tau + wrench)", cid, 2000),
                (f"inverse_dynamics + rb refresh + torch ADMM, {D_['iters']} iterations", compose, 5)]
    for _nm, f, _c in variants:
        for _ in range(2):
            f()
    qp(D_["iters"])()
    torch.cuda.synchronize()
    diff = float((res["z"] - forces.view(N, 4 * K, 3)).abs().max())
    lines = [f"  largest force {float(forces.abs().max()):.1f} N, loaded vertices per env "
             f"{float(info[:, 3].mean()):.2f}, |tau[0:3]| mean {float(info[:, 0].mean()):.2f} N; "
             f"|composition - kernel| max force {diff:.2e} N"]
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
    out = [f"N = {N}, thormang, K = {K} soles; HIP events around blocks of back-to-back calls, {BLOCKS} alternating "
           "blocks, median (min-max) per call"] + lines
    for nm, _, calls in variants:
        t = times[nm]
        out.append(f"  {nm:72s} {statistics.median(t):9.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
                   f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
