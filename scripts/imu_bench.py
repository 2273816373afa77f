"""Developer micro-benchmark of the IMU (tg_imu) at 4096 envs:

    thormang  S = 1 (imu_link)
    thormang  S = 3 (imu_link and both feet)
    gogoro    S = 1 (the root link)

each against the same readings composed in torch on the same device from the
refreshed rigid-body state tensor and a kept previous-velocity tensor (the
link's quaternion to a rotation, the com velocity moved to the sensor point,
the projected gravity, the body-frame velocities, the differenced
accelerations, the 20 slots stacked, the previous velocities stored), and
beside tg_height_scan with the same frames and one pattern point on the same
sim, which shares the forward kinematics.  The fused call is timed through
Sim.imu and through the C entry with prebuilt arguments: where Python's
argument checks take longer than the kernel, only the latter shows the device.
The largest difference between the kernel's and the composition's readings is
printed, relative to the largest reading of each slot group.

HIP events around blocks of back-to-back calls (2000 of a fused call, 200 of a
composition), seven alternating blocks, median (min-max) per call; the host
time to enqueue a call is printed too, so a figure that is the enqueue rate and
not the device's duration can be told apart.  No GPU, no figure: the script
fails without one.

    python scripts/imu_bench.py
"""
import ctypes as C
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from thormang_isaacgym_amd import abi  # noqa: E402
from thormang_isaacgym_amd._lib import lib  # noqa: E402
from thormang_isaacgym_amd.sim import Sim, load_model  # noqa: E402

N, BLOCKS, DT = 4096, 7, 0.01
G = (0.0, 0.0, -9.81)


def quat_to_R(q):
    """[..., 4] xyzw -> [..., 3, 3]"""
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)],
                       dim=-1).unflatten(-1, (3, 3))


def make_sim(name):
    dev = "cuda:0"
    m = load_model(name)
    sp = abi.sim_params_from_cfg({"dt": DT, "substeps": 1, "gravity": list(G)}, {}, N)
    s = Sim(m, sp, N, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    s.root_state[:, :2] = torch.rand(N, 2, device=dev, generator=g) * 90.0
    s.root_state[:, 2] = 1.0
    q = torch.randn(N, 4, device=dev, generator=g)
    s.root_state[:, 3:7] = q / q.norm(dim=1, keepdim=True)
    s.root_state[:, 7:13] = torch.randn(N, 6, device=dev, generator=g)
    s.dof_state[:, 0] = torch.rand(N * s.D, device=dev, generator=g) * 0.4 - 0.2
    s.dof_state[:, 1] = torch.randn(N * s.D, device=dev, generator=g)
    s.refresh()
    return m, s


class Setup:
    """One sim with its sensors: the fused call, the torch composition and the height scan beside them."""

    def __init__(self, label, m, s, links):
        dev = "cuda:0"
        self.label, self.s, S = label, s, len(links)
        self.sensors = [s.contact_frame(l) for l in links]
        self.links = torch.tensor(links, device=dev)
        self.com = torch.as_tensor(abi.model_arrays(m)["link_inertia"][links, 1:4], dtype=torch.float32, device=dev)
        self.rb = s.acquire_rigid_body_state_tensor().view(N, s.L, 13)
        self.hist, self.out = s.imu_history(S), torch.zeros(N, S, abi.TG_IMU_WIDTH, device=dev)
        self.prev = torch.zeros(N, S, 6, device=dev)
        self.prev_valid = torch.zeros(N, S, device=dev)
        self.g = torch.tensor(G, device=dev)
        self.point = torch.zeros(1, 2, device=dev)
        self.heights = torch.zeros(N, S, 1, device=dev)
        self.composed = None
        # the C entry with its arguments built once: the device's duration where Sim.imu's Python is the slower
        self._ip = abi.tg_imu_params()
        self._ip.dt = DT
        self._arr = (abi.tg_contact_frame * S)(*self.sensors)
        self._args = (s.handle, self._arr, S, C.byref(self._ip), None, None, C.c_void_p(self.hist.data_ptr()),
                      C.c_void_p(self.out.data_ptr()))

    def fused(self):
        self.s.imu(self.sensors, history=self.hist, dt=DT, out=self.out)

    def fused_c(self):
        lib().tg_imu(*self._args)

    def scan(self):
        self.s.height_scan(self.sensors, self.point, out=self.heights)

    def torch_composition(self):
        self.s.refresh_rigid_body_state_tensor()
        row = self.rb[:, self.links]
        q, vc, w = row[..., 3:7], row[..., 7:10], row[..., 10:13]
        R = quat_to_R(q)
        v = vc + torch.cross(w, (R @ (-self.com)[None, :, :, None]).squeeze(-1), dim=-1)   # com -> link origin
        Rt = R.transpose(-1, -2)
        valid = self.prev_valid
        a = (v - self.prev[..., 0:3]) / DT * valid[..., None]
        alpha = (w - self.prev[..., 3:6]) / DT * valid[..., None]

        def body(x):
            return (Rt @ x[..., None]).squeeze(-1)
        gb = body((self.g / self.g.norm()).expand_as(v))
        self.composed = torch.cat([q, gb, body(v), body(w), body(a - self.g), body(alpha), valid[..., None]], dim=-1)
        self.prev[..., 0:3] = v
        self.prev[..., 3:6] = w
        self.prev_valid.fill_(1.0)

    def difference(self):
        """Seed both at the current state, move the velocities, read both: the largest difference per slot group
        relative to the group's largest reading."""
        s = self.s
        self.hist.zero_()
        self.prev_valid.zero_()
        self.fused()
        self.torch_composition()
        g = torch.Generator(device="cuda:0").manual_seed(3)
        s.root_state[:, 7:13] += 0.1 * torch.randn(N, 6, device="cuda:0", generator=g)
        s.dof_state[:, 1] += 0.1 * torch.randn(N * s.D, device="cuda:0", generator=g)
        self.fused()
        self.torch_composition()
        torch.cuda.synchronize()
        a, b = self.out.double(), self.composed.double()
        sign = torch.where((a[..., 0:4] * b[..., 0:4]).sum(-1, keepdim=True) < 0, -1.0, 1.0)
        b = torch.cat([b[..., 0:4] * sign, b[..., 4:]], dim=-1)
        fig = {}
        for name, lo, hi in (("quat", 0, 4), ("gravity", 4, 7), ("velocities", 7, 13), ("accelerations", 13, 19)):
            fig[name] = float((a[..., lo:hi] - b[..., lo:hi]).abs().max() / b[..., lo:hi].abs().max())
        assert bool((a[..., 19] == 1).all()) and bool((b[..., 19] == 1).all())
        return fig


def main():
    assert torch.cuda.is_available(), "imu_bench needs the MI355X"
    mt, st = make_sim("thormang")
    mg, sg = make_sim("gogoro")
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
    imu = mt.link_index("imu_link")
    setups = [Setup("thormang S=1 (imu_link)", mt, st, [imu]),
              Setup("thormang S=3 (imu_link, feet)", mt, st, [imu] + walk_feet_indices(mt)),
              Setup("gogoro S=1 (root)", mg, sg, [0])]
    variants = []
    for u in setups:
        variants += [(f"{u.label} Sim.imu", u.fused, 2000),
                     (f"{u.label} tg_imu, C entry", u.fused_c, 2000),
                     (f"{u.label} tg_height_scan, P = 1", u.scan, 2000),
                     (f"{u.label} rb refresh + torch composition", u.torch_composition, 200)]
    for _, f, _n in variants:                                 # warm every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    print(f"N = {N}, dt = {DT}; |composition - kernel| / max |reading| per slot group:")
    for u in setups:
        print(f"  {u.label:32s} " + ", ".join(f"{k} {v:.2e}" for k, v in u.difference().items()))
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
        print(f"  {nm:64s} {statistics.median(t):8.1f} us ({min(t):.1f}-{max(t):.1f})   host enqueue "
              f"{statistics.median(host[nm]):.1f} us/call, {calls} calls per block")
    print(f"  bytes per launch: out S=1 {N * 80}, S=3 {N * 240}; history read and written S=1 {N * 32}, S=3 {N * 96}")


if __name__ == "__main__":
    main()
