"""Developer micro-benchmark of the capsule proximity (tg_proximity) at 4096
envs:

    thormang  the walk's default set (walk_self_capsules, Sim.capsule_pairs:
              15 capsules, 99 pairs): summary only, dist only, all three outputs
    gogoro    six capsules -- the rider's forearms and hands against the
              scooter's head and body links, 8 pairs -- all three outputs

Next to each: tg_height_scan about the capsules' links with one point each (the
floor: the same forward kinematics and a handful of stores; the scan takes eight
frames, so the first eight links stand for the set -- the forward kinematics
runs over the whole tree whatever the frames), and the same distances and
summary composed in torch from refresh_rigid_body_state_tensor.  The largest
difference between the composition and the kernel is printed.

The kernel and the scan are called through the C function with their argument
arrays built once, so that the figure is the launch and not the wrapper; the
wrapper's own host time per call (Sim.proximity builds the arrays from its
arguments every call) is printed beside it.  HIP events around blocks of
back-to-back calls, seven alternating blocks, median (min-max) per call.  No
GPU, no figure: the script fails without one.

    python scripts/proximity_bench.py [--out profiles/r12/proximity_timing.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd._lib import check, lib  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402
from thormang_isaacgym_amd.tasks.thormang_walk import WALK_SELF_MARGIN, walk_self_capsules  # noqa: E402

N, BLOCKS = 4096, 7


def quat_rotate(q, v):
    """q [N, C, 4] xyzw applied to v [C, 3] -> [N, C, 3]."""
    qv, w = q[..., :3], q[..., 3:4]
    v = v[None].expand(q.shape[0], -1, -1)
    t = 2.0 * torch.cross(qv, v, dim=-1)
    return v + w * t + torch.cross(qv, t, dim=-1)


def torch_proximity(rb, links, p0, p1, rad, ia, ib, margin):
    """dist [N, P] and summary [N, 4] composed from the rigid-body states rb [N, L, 13]: Ericson's clamped
    closest points, vectorised over envs and pairs."""
    pos, q = rb[:, links, :3], rb[:, links, 3:7]
    a0, a1 = pos + quat_rotate(q, p0), pos + quat_rotate(q, p1)
    pa, pb = a0[:, ia], a0[:, ib]
    d1, d2 = a1[:, ia] - pa, a1[:, ib] - pb
    r = pa - pb
    a, e, f = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d2 * r).sum(-1)
    c, b = (d1 * r).sum(-1), (d1 * d2).sum(-1)
    one = torch.ones_like(a)
    sa, se = torch.where(a > 1e-12, a, one), torch.where(e > 1e-12, e, one)
    den = a * e - b * b
    s = torch.where((den > 0) & (a > 1e-12), ((b * f - c * e) / torch.where(den > 0, den, one)).clamp(0, 1), 0 * a)
    t = torch.where(e > 1e-12, (b * s + f) / se, 0 * e)
    tc = t.clamp(0, 1)
    s = torch.where((t != tc) & (a > 1e-12), ((b * tc - c) / sa).clamp(0, 1), s)
    sep = (pa + s[..., None] * d1) - (pb + tc[..., None] * d2)
    dist = sep.norm(dim=-1) - rad[ia] - rad[ib]
    best, first = dist.min(dim=1)
    summary = torch.stack([best, first.float(), (dist < margin).sum(1).float(), (margin - dist).clamp(min=0).sum(1)], 1)
    return dist, summary


def make_sim(name):
    dev = "cuda:0"
    m = load_model(name)
    sp = abi.sim_params_from_cfg({"dt": 0.01, "substeps": 1, "gravity": [0.0, 0.0, -9.81]}, {}, N)
    s = Sim(m, sp, N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :2] = torch.rand(N, 2, device=dev, generator=g) * 90.0
    s.root_state[:, 2] = 1.0
    q = torch.randn(N, 4, device=dev, generator=g) * 0.08
    yaw = torch.rand(N, device=dev, generator=g) * 6.2832
    q[:, 2], q[:, 3] = torch.sin(yaw / 2), torch.cos(yaw / 2)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 0.8 - 0.4
    s.refresh()
    return m, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "proximity_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "proximity_bench needs the MI355X"
    dev = "cuda:0"
    mt, st = make_sim("thormang")
    mg, sg = make_sim("gogoro")
    walk = walk_self_capsules(mt)
    six = [sg.limb_capsule(f"{x}_arm_el_y_link", f"{x}_arm_wr_r_link", 0.045) for x in "lr"] + \
          [sg.limb_capsule(f"{x}_arm_wr_p_link", f"{x}_arm_end_link", 0.04) for x in "lr"] + \
          [sg.capsule("head", (0.0, 0.0, -0.2), (0.0, 0.0, 0.3), 0.05),
           sg.capsule("body", (-0.4, 0.0, 0.1), (0.3, 0.0, 0.1), 0.12)]
    configs = [   # name, sim, capsules, pairs, outputs, calls per block
        ("thormang 15 capsules, 99 pairs: summary", st, walk, st.capsule_pairs(walk), "s", 2000),
        ("thormang 15 capsules, 99 pairs: dist", st, walk, st.capsule_pairs(walk), "d", 2000),
        ("thormang 15 capsules, 99 pairs: dist, witness, summary", st, walk, st.capsule_pairs(walk), "dws", 2000),
        ("gogoro 6 capsules, 8 pairs: dist, witness, summary", sg, six, [(a, b) for a in range(4) for b in (4, 5)],
         "dws", 2000),
    ]
    lines, variants, keep = [], [], []
    for name, s, caps, pairs, outs, calls in configs:
        Cn, P = len(caps), len(pairs)
        dist, wit, summ = (torch.zeros(N, P, device=dev), torch.zeros(N, P, 6, device=dev),
                           torch.zeros(N, 4, device=dev))
        arr = (abi.tg_capsule * Cn)(*caps)
        idx = (C.c_int32 * (2 * P))(*[v for ab in pairs for v in ab])
        pp = abi.tg_proximity_params()
        pp.margin = WALK_SELF_MARGIN
        ptrs = [C.c_void_p(t.data_ptr()) if k in outs else None for k, t in zip("dws", (dist, wit, summ))]
        links = sorted({int(c.link) for c in caps})[:abi.TG_SCAN_MAX_FRAMES]
        frames = (abi.tg_contact_frame * len(links))(*[s.contact_frame(l) for l in links])
        point = torch.zeros(1, 2, device=dev)
        heights = torch.zeros(N, len(links), 1, device=dev)
        spar = abi.tg_scan_params()
        spar.surface, spar.align = abi.TG_SCAN_SURFACE, abi.TG_SCAN_YAW
        rb = s.acquire_rigid_body_state_tensor().view(N, s.L, 13)
        tl = torch.tensor([int(c.link) for c in caps], device=dev)
        tp0 = torch.tensor([list(c.p0) for c in caps], device=dev)
        tp1 = torch.tensor([list(c.p1) for c in caps], device=dev)
        trad = torch.tensor([c.radius for c in caps], device=dev)
        tia = torch.tensor([a for a, _b in pairs], device=dev)
        tib = torch.tensor([b for _a, b in pairs], device=dev)
        keep.append((arr, idx, pp, frames, point, spar))
        res = {}

        def prox(s=s, arr=arr, Cn=Cn, idx=idx, P=P, pp=pp, ptrs=ptrs):
            check(lib().tg_proximity(s.handle, arr, Cn, idx, P, C.byref(pp), *ptrs), "proximity")

        def wrapper(s=s, caps=caps, pairs=pairs, outs=outs, dist=dist, wit=wit, summ=summ):
            s.proximity(caps, pairs, margin=WALK_SELF_MARGIN, dist="d" in outs, witness="w" in outs,
                        summary="s" in outs, out=dist, out_witness=wit, out_summary=summ)

        def scan(s=s, frames=frames, F=len(links), point=point, spar=spar, heights=heights):
            check(lib().tg_height_scan(s.handle, frames, F, C.c_void_p(point.data_ptr()), 1, C.byref(spar),
                                       C.c_void_p(heights.data_ptr()), None), "height_scan")

        def compose(s=s, rb=rb, res=res, a=(tl, tp0, tp1, trad, tia, tib)):
            s.refresh_rigid_body_state_tensor()
            res["d"], res["s"] = torch_proximity(rb, *a, WALK_SELF_MARGIN)

        variants += [(f"{name}: tg_proximity", prox, calls), (f"{name}: Sim.proximity (wrapper)", wrapper, calls),
                     (f"{name}: tg_height_scan, {len(links)} frames x 1 point", scan, calls),
                     (f"{name}: rb refresh + torch composition", compose, 50)]
        for f in (prox, wrapper, scan, compose):
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        check(lib().tg_proximity(s.handle, arr, Cn, idx, P, C.byref(pp), C.c_void_p(dist.data_ptr()), None,
                                 C.c_void_p(summ.data_ptr())), "proximity")
        torch.cuda.synchronize()
        lines.append(f"  {name}: min dist {float(dist.min()):.4f}, envs with a pair under the margin "
                     f"{float((summ[:, 2] > 0).float().mean()):.3f}; |composition - kernel| max dist "
                     f"{float((res['d'] - dist).abs().max()):.2e}, summary[3] "
                     f"{float((res['s'][:, 3] - summ[:, 3]).abs().max()):.2e}")
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
    out = [f"N = {N}; HIP events around blocks of back-to-back calls, {BLOCKS} alternating blocks, median (min-max) "
           "per call"] + lines
    for nm, _, calls in variants:
        t = times[nm]
        out.append(f"  {nm:84s} {statistics.median(t):9.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
                   f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
