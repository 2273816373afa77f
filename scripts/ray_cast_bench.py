"""Developer micro-benchmark of the ray cast (tg_ray_cast) at 4096 envs on a
512 x 512 heightfield with hs = 0.25:

    thormang  a 96-ray lidar (16 azimuths x 6 elevations) at lidar_link, range 10 m
    gogoro    the 32 x 24 depth image of env.enableDepthCamera at realsense_link
    gogoro    the 64 x 48 image at realsense_link (hfov 87 degrees, depth bound 8 m)

Next to each: tg_height_scan with the same frames and as many samples (the
floor: forward kinematics plus one lookup per sample; 3072 samples are three
copies of the frame x 1024 points, the scan's limit per frame), the mean number
of heightfield cells a ray walks (counted here from the geometry: the cells
between the point where the clipped ray comes under the highest vertex over the
grid and the point where it ends), and the cast composed in torch: the frame
from refresh_rigid_body_state_tensor, a fixed-step march at hs / 2 along each
ray against ground_at restated in torch, and one bisection refinement.  The
largest difference between the composition and the kernel is printed with the
share of rays over 2 cm (the march steps over thin ridges; it is the cost that
is compared, not the result).

HIP events around blocks of back-to-back calls, seven alternating blocks, median
(min-max) per call; the host time to enqueue a call is printed too.  No GPU, no
figure: the script fails without one.

    python scripts/ray_cast_bench.py [--out profiles/r10/ray_cast_timing.txt]
"""
import argparse
import os
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


def torch_ground(hf, x, y):
    """max(H, 0) of ground_at in torch."""
    u, v = (x - OX) / HS, (y - OY) / HS
    on = (u >= 0) & (v >= 0) & (u <= ROWS - 1) & (v <= COLS - 1)
    i = torch.clip(u.long(), 0, ROWS - 2)
    j = torch.clip(v.long(), 0, COLS - 2)
    fu, fv = u - i, v - j
    h00, h01, h10, h11 = VS * hf[i, j], VS * hf[i, j + 1], VS * hf[i + 1, j], VS * hf[i + 1, j + 1]
    low = fu >= fv
    gx, gy = torch.where(low, h10 - h00, h11 - h01), torch.where(low, h11 - h10, h01 - h00)
    H = h00 + fu * gx + fv * gy
    return torch.where(on & (H > 0), H, torch.zeros_like(H))


def quat_rotate(q, v):
    """q [N, 4] xyzw applied to v [R, 3] -> [N, R, 3]."""
    qv, w = q[:, None, :3], q[:, None, 3:4]
    v = v[None]
    t = 2.0 * torch.cross(qv.expand(-1, v.shape[1], -1), v.expand(q.shape[0], -1, -1), dim=-1)
    return v + w * t + torch.cross(qv.expand_as(t), t, dim=-1)


def world_rays(rb_link, rays):
    """(o, d) [N, R, 3] of the pattern in the link's axes at the link's pose rb_link [N, 13]."""
    q = rb_link[:, 3:7]
    return rb_link[:, None, :3] + quat_rotate(q, rays[:, :3]), quat_rotate(q, rays[:, 3:])


def torch_cast(hf, o, d, max_range):
    """A fixed-step marcher at hs / 2 (in metres along the ray) with one bisection refinement."""
    dn = d.norm(dim=-1)
    step = 0.5 * HS / dn                                     # in t
    steps = int(float((max_range * dn).max()) / (0.5 * HS)) + 1
    dist = torch.full_like(dn, max_range)
    found = torch.zeros_like(dn, dtype=torch.bool)
    for k in range(1, steps + 1):
        t = torch.clamp(k * step, max=max_range)
        p = o + t[..., None] * d
        inside = p[..., 2] <= torch_ground(hf, p[..., 0], p[..., 1])
        new = inside & ~found
        tm = t - 0.5 * step                                  # one bisection step
        pm = o + tm[..., None] * d
        mid_in = pm[..., 2] <= torch_ground(hf, pm[..., 0], pm[..., 1])
        dist = torch.where(new, torch.where(mid_in, tm - 0.25 * step, tm + 0.25 * step), dist)
        found |= new
    return torch.where(dist < max_range, dist, torch.full_like(dist, max_range))


def cells_walked(o, d, dist, zcap):
    """Mean number of cells a ray's walk touches: from where the ray, clipped to the grid and to z <= zcap, starts
    to where it ends (its hit, or the end of the clipped span)."""
    U0, V0, dU, dV = (o[..., 0] - OX) / HS, (o[..., 1] - OY) / HS, d[..., 0] / HS, d[..., 1] / HS
    big = torch.full_like(U0, 3.0e38)
    t0, t1 = torch.zeros_like(U0), dist.clone()
    for p0, dp, top in ((U0, dU, ROWS - 1.0), (V0, dV, COLS - 1.0)):
        safe = torch.where(dp != 0, dp, torch.ones_like(dp))
        ta, tb = (0.0 - p0) / safe, (top - p0) / safe
        lo, hi = torch.minimum(ta, tb), torch.maximum(ta, tb)
        outside = (p0 < 0) | (p0 > top)
        t0 = torch.where(dp != 0, torch.maximum(t0, lo), t0)
        t1 = torch.where(dp != 0, torch.minimum(t1, hi), torch.where(outside, -big, t1))
    dz = d[..., 2]
    safe = torch.where(dz != 0, dz, torch.ones_like(dz))
    tz = (zcap - o[..., 2]) / safe
    t0 = torch.where(dz < 0, torch.maximum(t0, tz), t0)
    t1 = torch.where(dz > 0, torch.minimum(t1, tz), torch.where((dz == 0) & (o[..., 2] > zcap), -big, t1))
    walks = t0 < t1
    t0, t1 = torch.where(walks, t0, torch.zeros_like(t0)), torch.where(walks, t1, torch.zeros_like(t1))
    n = (torch.floor(U0 + t1 * dU) - torch.floor(U0 + t0 * dU)).abs() + \
        (torch.floor(V0 + t1 * dV) - torch.floor(V0 + t0 * dV)).abs() + 1
    return float(torch.where(walks, n, torch.zeros_like(n)).mean()), float(walks.float().mean())


def make_sim(name, hf_np):
    dev = "cuda:0"
    m = load_model(name)
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0.0, 0.0, -9.81]}, {}, N)
    s = Sim(m, sp, N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :2] = torch.rand(N, 2, device=dev, generator=g) * 90.0      # over the 127 m terrain
    s.root_state[:, 2] = 1.0
    q = torch.randn(N, 4, device=dev, generator=g) * 0.08                       # nearly upright, any heading
    yaw = torch.rand(N, device=dev, generator=g) * 6.2832
    q[:, 2], q[:, 3] = torch.sin(yaw / 2), torch.cos(yaw / 2)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 0.4 - 0.2
    s.refresh()
    s.set_heightfield(hf_np, HS, VS, OX, OY)
    return m, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "ray_cast_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ray_cast_bench needs the MI355X"
    dev = "cuda:0"
    rs = np.random.default_rng(2)
    i, j = np.meshgrid(np.arange(ROWS) * HS, np.arange(COLS) * HS, indexing="ij")
    z = sum(np.sin(rs.uniform(0.8, 2.0) * (np.cos(a) * i + np.sin(a) * j) + rs.uniform(0, 6.28))
            for a in rs.uniform(0, 6.28, 4))
    hf_np = np.round((0.3 * z / np.abs(z).max() + 0.08) / VS).astype(np.float32)
    zcap = float((VS * hf_np).max())
    hf = torch.from_numpy(hf_np).to(dev)
    mg, sg = make_sim("gogoro", hf_np)
    mt, st = make_sim("thormang", hf_np)
    lidar = st.lidar_rays(np.deg2rad(3.0 + 22.5 * np.arange(16)), np.deg2rad([-50.0, -30.0, -15.0, -7.0, -2.0, 8.0]))
    hfov = np.deg2rad(87.0)
    configs = [   # name, sim, model, link, rays, max_range, calls per block (kernel, composition)
        ("thormang lidar 96 @ lidar_link", st, mt, "lidar_link", lidar, 10.0, 2000, 20),
        ("gogoro depth 32 x 24 @ realsense_link", sg, mg, "realsense_link", sg.pinhole_rays(32, 24, hfov), 8.0, 500, 5),
        ("gogoro depth 64 x 48 @ realsense_link", sg, mg, "realsense_link", sg.pinhole_rays(64, 48, hfov), 8.0, 200, 3),
    ]
    lines, variants, res = [], [], {}
    for name, s, m, link, rays, rng, calls, calls_t in configs:
        l = m.link_index(link)
        R = rays.shape[0]
        frame = [s.contact_frame(l)]
        dist = torch.zeros(N, 1, R, device=dev)
        copies = (R + abi.TG_SCAN_MAX_POINTS - 1) // abi.TG_SCAN_MAX_POINTS
        P = R // copies
        assert P * copies == R
        pts = (torch.rand(P, 2, device=dev) * 2.0 - 1.0).contiguous()
        heights = torch.zeros(N, copies, P, device=dev)
        rb = s.acquire_rigid_body_state_tensor().view(N, s.L, 13)

        def cast(s=s, frame=frame, rays=rays, rng=rng, dist=dist):
            s.ray_cast(frame, rays, align="link", max_range=rng, out=dist)

        def scan(s=s, frame=frame, copies=copies, pts=pts, heights=heights):
            s.height_scan(frame * copies, pts, out=heights)

        def compose(s=s, rb=rb, l=l, rays=rays, rng=rng, name=name):
            s.refresh_rigid_body_state_tensor()
            o, d = world_rays(rb[:, l], rays)
            res[name] = torch_cast(hf, o, d, rng)

        variants += [(f"{name}: tg_ray_cast", cast, calls),
                     (f"{name}: tg_height_scan, {copies} x {P} samples", scan, calls),
                     (f"{name}: rb refresh + torch march", compose, calls_t)]
        for f in (cast, scan, compose):                         # warm every shape
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        s.refresh_rigid_body_state_tensor()
        torch.cuda.synchronize()
        o, d = world_rays(rb[:, l], rays)
        cells, share = cells_walked(o, d, dist[:, 0], zcap)
        diff = (res[name] - dist[:, 0]).abs()
        hit = float((dist < rng).float().mean())
        lines.append(f"  {name}: R = {R}, rays per launch {N * R}, hits {hit:.3f}, rays that walk {share:.3f}, mean "
                     f"cells per ray, estimated from the geometry, {cells:.2f}; |march - kernel| max {float(diff.max()):.2e}, share over 0.02: "
                     f"{float((diff > 0.02).float().mean()):.2e}")
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
    out = [f"N = {N}, heightfield {ROWS} x {COLS}, hs = {HS}; HIP events around blocks of back-to-back calls, "
           f"{BLOCKS} alternating blocks, median (min-max) per call"] + lines
    for nm, _, calls in variants:
        t = times[nm]
        out.append(f"  {nm:64s} {statistics.median(t):10.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
                   f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
