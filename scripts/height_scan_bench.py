"""Developer micro-benchmark of the height scan (tg_height_scan) at 4096 envs on
a 512 x 512 heightfield, the reference's 140-point pattern, yaw aligned:

    gogoro    F = 1 (the root link)          cell rule and surface rule
    thormang  F = 3 (the root and both feet) surface rule, with normals too

each against the same scan composed in torch on the same device: the
reference's get_heights (tasks/anymal_terrain.py:513-536: quat_apply_yaw, two
advanced-index gathers, min) for the cell rule, and ground_at restated in torch
(four gathers, the triangle rule, the plane) for the surface rule; for frames
that are not the root, refresh_rigid_body_state_tensor first.  The largest
difference between the two results is printed (samples on a cell line or a
diagonal may take the other side in one of them).

HIP events around blocks of back-to-back calls (2000 of a fused call, 200 of a
composition), seven alternating blocks, median (min-max) per call; the host
time to enqueue a call is printed too, so a figure that is the enqueue rate and
not the device's duration can be told apart.  No GPU, no figure: the script
fails without one.

    python scripts/height_scan_bench.py
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
ROWS = COLS = 512
HS, VS, OX, OY = 0.25, 0.005, -30.0, -30.0


def quat_apply_yaw_xy(q, pts):
    """The x, y of the reference's quat_apply_yaw(q, (a, b, 0)): q [..., 4] xyzw, pts [P, 2] -> [..., P, 2]."""
    z, w = q[..., 2], q[..., 3]
    n = torch.sqrt(z * z + w * w)
    z, w = z / n, w / n
    c, s = (w * w - z * z)[..., None], (2 * w * z)[..., None]
    return torch.stack([c * pts[:, 0] - s * pts[:, 1], s * pts[:, 0] + c * pts[:, 1]], dim=-1)


def torch_cell(hf, x, y):
    px = torch.clip(((x - OX) / HS).long(), 0, ROWS - 2)
    py = torch.clip(((y - OY) / HS).long(), 0, COLS - 2)
    return torch.min(hf[px, py], hf[px + 1, py + 1]) * VS


def torch_surface(hf, x, y):
    """ground_at in torch: (h, n)"""
    u, v = (x - OX) / HS, (y - OY) / HS
    on = (u >= 0) & (v >= 0) & (u <= ROWS - 1) & (v <= COLS - 1)
    i = torch.clip(u.long(), 0, ROWS - 2)
    j = torch.clip(v.long(), 0, COLS - 2)
    fu, fv = u - i, v - j
    h00, h01, h10, h11 = VS * hf[i, j], VS * hf[i, j + 1], VS * hf[i + 1, j], VS * hf[i + 1, j + 1]
    low = fu >= fv
    gx, gy = torch.where(low, h10 - h00, h11 - h01), torch.where(low, h11 - h10, h01 - h00)
    H = h00 + fu * gx + fv * gy
    t = on & (H > 0)
    sx, sy = gx / HS, gy / HS
    inv = torch.rsqrt(sx * sx + sy * sy + 1)
    zero = torch.zeros_like(H)
    n = torch.stack([torch.where(t, -sx * inv, zero), torch.where(t, -sy * inv, zero),
                     torch.where(t, inv, zero + 1)], dim=-1)
    return torch.where(t, H, zero), n


def make_sim(name, hf_np):
    dev = "cuda:0"
    m = load_model(name)
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0.0, 0.0, -9.81]}, {}, N)
    s = Sim(m, sp, N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :2] = torch.rand(N, 2, device=dev, generator=g) * 90.0      # over the 127 m terrain
    s.root_state[:, 2] = 1.0
    q = torch.randn(N, 4, device=dev, generator=g)
    q[:, 3] += 2.0                                                              # (headings well conditioned)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 0.4 - 0.2
    s.refresh()
    s.set_heightfield(hf_np, HS, VS, OX, OY)
    return m, s


def main():
    assert torch.cuda.is_available(), "height_scan_bench needs the MI355X"
    dev = "cuda:0"
    rs = np.random.default_rng(2)
    i, j = np.meshgrid(np.arange(ROWS) * HS, np.arange(COLS) * HS, indexing="ij")
    z = sum(np.sin(rs.uniform(0.8, 2.0) * (np.cos(a) * i + np.sin(a) * j) + rs.uniform(0, 6.28))
            for a in rs.uniform(0, 6.28, 4))
    hf_np = np.round((0.3 * z / np.abs(z).max() + 0.08) / VS).astype(np.float32)
    hf = torch.from_numpy(hf_np).to(dev)
    _mg, sg = make_sim("gogoro", hf_np)
    mt, st = make_sim("thormang", hf_np)
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
    feet = walk_feet_indices(mt)
    links = torch.tensor([0] + feet, device=dev)
    pts = sg.scan_grid(0.1 * torch.tensor([-8, -7, -6, -5, -4, -3, -2, 2, 3, 4, 5, 6, 7, 8], dtype=torch.float32),
                       0.1 * torch.tensor([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], dtype=torch.float32))
    P = pts.shape[0]
    fg = [sg.contact_frame(0)]
    ft = [st.contact_frame(l) for l in [0] + feet]
    hg, ht, nt = (torch.zeros(N, 1, P, device=dev), torch.zeros(N, 3, P, device=dev),
                  torch.zeros(N, 3, P, 3, device=dev))
    rb = st.acquire_rigid_body_state_tensor().view(N, st.L, 13)
    res = {}

    def g_cell():
        sg.height_scan(fg, pts, surface="cell", out=hg)

    def g_cell_torch():
        r = sg.root_state
        xy = quat_apply_yaw_xy(r[:, 3:7], pts) + r[:, None, :2]
        res["g_cell"] = torch_cell(hf, xy[..., 0], xy[..., 1])

    def g_surface():
        sg.height_scan(fg, pts, out=hg)

    def g_surface_torch():
        r = sg.root_state
        xy = quat_apply_yaw_xy(r[:, 3:7], pts) + r[:, None, :2]
        res["g_surface"] = torch_surface(hf, xy[..., 0], xy[..., 1])[0]

    def t_surface():
        st.height_scan(ft, pts, out=ht)

    def t_normals():
        st.height_scan(ft, pts, normals=True, out=ht, out_normals=nt)

    def t_surface_torch():
        st.refresh_rigid_body_state_tensor()
        fr = rb[:, links]
        xy = quat_apply_yaw_xy(fr[..., 3:7], pts) + fr[:, :, None, :2]
        res["t_surface"], res["t_normals"] = torch_surface(hf, xy[..., 0], xy[..., 1])

    variants = [("gogoro F=1 tg_height_scan (cell)", g_cell, 2000),
                ("gogoro F=1 torch get_heights (cell)", g_cell_torch, 200),
                ("gogoro F=1 tg_height_scan (surface)", g_surface, 2000),
                ("gogoro F=1 torch ground_at (surface)", g_surface_torch, 200),
                ("thormang F=3 tg_height_scan (surface)", t_surface, 2000),
                ("thormang F=3 tg_height_scan (surface + normals)", t_normals, 2000),
                ("thormang F=3 rb refresh + torch ground_at (+ normals)", t_surface_torch, 200)]
    for _, f, _n in variants:                                 # warm every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()

    def agree(a, b_, tol=1e-4):
        d = (a - b_).abs()
        return f"max {float(d.max()):.2e}, share over {tol:g}: {float((d > tol).float().mean()):.2e}"

    g_cell()
    torch.cuda.synchronize()
    print(f"N = {N}, P = {P}, heightfield {ROWS} x {COLS}; |composition - kernel|: gogoro cell "
          f"{agree(res['g_cell'], hg[:, 0])}", end="; ")
    g_surface()
    t_normals()
    torch.cuda.synchronize()
    print(f"gogoro surface {agree(res['g_surface'], hg[:, 0])}; thormang surface {agree(res['t_surface'], ht)}; "
          f"thormang normals {agree(res['t_normals'], nt)}")
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
        print(f"  {nm:56s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
              f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    print(f"  bytes written per launch: heights F=1 {N * P * 4}, F=3 {N * 3 * P * 4}, normals F=3 {N * 3 * P * 12}; "
          f"the heightfield {ROWS * COLS * 4}")


if __name__ == "__main__":
    main()
