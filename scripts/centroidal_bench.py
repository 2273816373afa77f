"""Developer micro-benchmark of the centroidal quantities (tg_centroidal) at
4096 envs on Thormang: three fused calls, each against the composition a user
had before it that computes the same numbers (the largest difference between
the two results is printed):

    state only   refresh_rigid_body_state_tensor + torch (link coms and world
                 inertias from the quaternions, the sums over the links)
    matrix       refresh_mass_matrix_tensors + the torch shift of its base rows
                 from the root link's com to the whole-body com (the lever arm
                 read off the matrix's own [0:3, 3:6] block)
    bias         inverse_dynamics(gravity=False) + the same shift of its base
                 rows, whose lever arm needs the com: the rigid-body-state
                 refresh and the torch com sum

HIP events around blocks of back-to-back calls (2000 of a fused call, 200 of a
composition, so that every window is tens of milliseconds), seven alternating
blocks, median (min-max) per call; the host time to enqueue a call is printed
too, so a figure that is the enqueue rate and not the device's duration can be
told apart.  No GPU, no figure: the script fails without one.

    python scripts/centroidal_bench.py
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


def quat_to_R(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(*q.shape[:-1], 3, 3)


def main():
    assert torch.cuda.is_available(), "centroidal_bench needs the MI355X"
    m = load_model("thormang")
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0.0, 0.0, -9.81]}, {}, N)
    s = Sim(m, sp, N, "cuda:0")
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :3] = torch.randn(N, 3, device=dev, generator=g)
    q = torch.randn(N, 4, device=dev, generator=g)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.root_state[:, 7:13] = torch.randn(N, 6, device=dev, generator=g)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 2 - 1
    s.dof_state[:, 1] = torch.randn(N * s.D, device=dev, generator=g)
    s.refresh()
    D, L = s.D, s.L
    li = torch.from_numpy(np.asarray(abi.model_arrays(m)["link_inertia"], np.float32).copy()).to(dev)
    mass, com = li[:, 0], li[:, 1:4]                                           # (unit mass scales)
    xx, yy, zz, xy, xz, yz = li[:, 4:10].unbind(-1)
    Il = torch.stack([xx, xy, xz, xy, yy, yz, xz, yz, zz], dim=-1).reshape(L, 3, 3)
    eye = torch.eye(3, device=dev)
    rb = s.acquire_rigid_body_state_tensor().view(N, L, 13)
    H = s.acquire_mass_matrix_tensor()
    st, A, b = (torch.zeros(N, 16, device=dev), torch.zeros(N, 6, 6 + D, device=dev), torch.zeros(N, 6, device=dev))
    tau = torch.zeros(N, 6 + D, device=dev)
    res = {}

    def fused_state():
        s.centroidal(out=st)

    def fused_matrix():
        s.centroidal(matrix=True, out=st, out_matrix=A)

    def fused_bias():
        s.centroidal(bias=True, out=st, out_bias=b)

    def fused_all():
        s.centroidal(matrix=True, bias=True, out=st, out_matrix=A, out_bias=b)

    def link_coms():
        R = quat_to_R(rb[:, :, 3:7])
        return R, rb[:, :, :3] + torch.einsum("elij,lj->eli", R, com)

    def torch_state():
        s.refresh_rigid_body_state_tensor()
        R, cl = link_coms()
        v, w = rb[:, :, 7:10], rb[:, :, 10:13]
        M = mass.sum()
        c = torch.einsum("l,eli->ei", mass, cl) / M
        cd = torch.einsum("l,eli->ei", mass, v) / M
        d = cl - c[:, None]
        Iw = R @ Il[None] @ R.transpose(-1, -2)
        k = (torch.einsum("elij,elj->ei", Iw, w) + torch.cross(d, mass[None, :, None] * v, dim=-1).sum(1))
        IG = (Iw + mass[None, :, None, None] * ((d * d).sum(-1)[..., None, None] * eye - d[..., :, None] * d[..., None, :])).sum(1)
        res["state"] = torch.cat([c, cd, k, M.expand(N, 1), IG[:, [0, 1, 2, 0, 0, 1], [0, 1, 2, 1, 2, 2]]], dim=1)

    def torch_matrix():
        s.refresh_mass_matrix_tensors()
        Mt = H[:, 0, 0]
        lever = torch.stack([H[:, 1, 5], -H[:, 0, 5], H[:, 0, 4]], dim=1) / Mt[:, None]      # c - c_root
        res["matrix"] = torch.cat([H[:, :3], H[:, 3:6] - torch.cross(lever[:, :, None].expand(N, 3, 6 + D), H[:, :3],
                                                                     dim=1)], dim=1)

    def torch_bias():
        s.inverse_dynamics(gravity=False, out=tau)
        s.refresh_rigid_body_state_tensor()
        R, cl = link_coms()
        lever = torch.einsum("l,eli->ei", mass, cl) / mass.sum() - cl[:, 0]
        res["bias"] = torch.cat([tau[:, :3], tau[:, 3:6] - torch.cross(lever, tau[:, :3], dim=1)], dim=1)

    variants = [("tg_centroidal (state only)", fused_state, 2000),
                ("rigid-body-state refresh + torch (state)", torch_state, 200),
                ("tg_centroidal (state + matrix)", fused_matrix, 2000),
                ("mass-matrix refresh + torch shift (matrix)", torch_matrix, 200),
                ("tg_centroidal (state + bias)", fused_bias, 2000),
                ("inverse_dynamics + rb refresh + torch shift (bias)", torch_bias, 200),
                ("tg_centroidal (all three)", fused_all, 2000)]
    for _, f, _n in variants:                                 # warm every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()

    def rel(a, b_):
        return float((a - b_).abs().max()) / float(b_.abs().max())

    print(f"thormang: N = {N}, D = {D}, L = {L}; max |composition - kernel| / max |kernel|: state "
          f"{rel(res['state'], st):.2e}, matrix {rel(res['matrix'], A):.2e}, bias {rel(res['bias'], b):.2e}")
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
        print(f"  {nm:52s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
              f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    print(f"  bytes written per env: state 64, matrix {6 * (6 + D) * 4}, bias 24; the rigid-body-state tensor "
          f"{L * 13 * 4}, the mass matrix {(6 + D) ** 2 * 4}")


if __name__ == "__main__":
    main()
