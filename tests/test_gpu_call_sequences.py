"""Call sequences against cache-free controls.

A training loop does not call the library in the canonical order create,
step, step, step: it interleaves DR setters, ``reset_idx``, force tensors,
tensor refreshes and re-bindings with the steps, in orders of its own.  Which
launches a step may skip is decided on the host from a handful of flags that
every entry point edits (``dirty_possible``, ``list_pending``, the shared
composite cache's ``cuni``, ``forces_pending`` / ``rbf_pending`` /
``rbf_prereduced``, the ``cf`` / ``df`` exports), so an entry point that
forgets one leaves a stale composite or wrench behind and nothing but the
next step's numbers would tell.

Every test here runs one scripted sequence on sim A (default environment)
and on the control B, created under the library's cache-free switches
(``TG_ALWAYS_COMPOSE``: every simulate composes; ``TG_NO_SHARED_CACHE``:
every env reads its own composite block), and requires ``torch.equal`` of
every state tensor after every simulate.  Bit equality is a condition, not a
tolerance: A and B launch the same step-kernel instantiation on the same
inputs, ``compose_env`` runs on the dirty envs only in both, and the shared
block is bitwise the env's own block whenever the flag says so.  (Controls
that swap in a differently compiled kernel -- ``TG_WALK_UNFUSED``,
``TG_POST_UNFUSED``, in-place seat updates against ``TG_SEAT_RECOMPOSE`` --
are held to 1e-5 by the tests of those paths and are not used here.)

So that no row passes vacuously, each asserts from ``tg_debug_launch_stats``
that A really took the cached path (composes skipped, list composes, the
``launch_rb_forces`` path, ...) and B did not; the rows marked C also run
the sequence without the write: the touched envs must differ from C and
every other env must equal it bit for bit (envs are independent).

24 envs: one full and one partial workgroup of 16 for both models; 16 where
the GogoroPaper one-launch step needs a multiple of 16."""
import pytest
import torch

from tests import call_sequences as cs

pytestmark = pytest.mark.gpu

N = 24


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _show(row, **stats):
    print(row, " ".join(f"{k}={v}" for k, v in stats.items()))


# ---------------------------------------------------------------- raw Sim rows
def _mass_write_run(monkeypatch, switches, ids, scale, write, recompose=False, pre=3, post=4):
    """``pre`` simulates, the mass write on ``ids`` (when ``write``; then
    optionally tg_composite(recompose=1)), ``post`` simulates.  Returns the
    trace and the launch statistics before and after the write."""
    sim = cs.create_under(monkeypatch, switches, lambda: cs.walk_sim(N))
    tg = cs.walk_targets(N, pre + post)
    trace = []
    for t in range(pre + post):
        if t == pre:
            before = cs.launch_stats(sim)
            if write:
                sim.set_body_mass_scale_indexed(cs.mass_rows(sim, ids, scale), cs.ids32(ids))
                if recompose:
                    cs.composite_recompose(sim)
        sim.set_dof_position_targets(tg[t])
        sim.simulate()
        trace.append(cs.snap_sim(sim))
    sim.sync()
    after = cs.since(sim, before)
    sim.close()
    return trace, before, after


def _check_against_c(trace_a, trace_c, ids, what):
    moved = cs.changed_envs(trace_a[-1], trace_c[-1], N)
    assert moved == set(ids), (what, "envs that differ from the run without the write", sorted(moved))


def test_gpu_r1_mass_write_between_simulates(monkeypatch):
    """R1: 3 simulates, set_body_mass_scale_indexed on one middle env (1.3 on
    every link), 4 simulates.  A composes once for the write and skips the
    compose before and after it; the control composes every time."""
    _cuda()
    ids = [N // 2]
    a, a0, a1 = _mass_write_run(monkeypatch, {}, ids, 1.3, True)
    b, b0, b1 = _mass_write_run(monkeypatch, cs.CONTROL, ids, 1.3, True)
    c, _, _ = _mass_write_run(monkeypatch, {}, ids, 1.3, False)
    _show("R1", A_before=a0, A_after=a1, B_before=b0, B_after=b1)
    cs.assert_same(a, b, "R1 A vs control")
    assert a0["full"] == 1 and a0["skipped"] == 2 and a1["full"] == 1 and a1["skipped"] == 3, (a0, a1)
    assert b0["skipped"] == 0 and b1["skipped"] == 0 and b1["full"] == 4, (b0, b1)
    _check_against_c(a, c, ids, "R1")


def test_gpu_r2_recompose_between_write_and_simulate(monkeypatch):
    """R2: R1 with tg_composite(recompose=1) between the write and the next
    simulate.  The re-compose clears ``dirty_possible``, so A skips every
    compose after the write: the shared-cache flag the step kernel reads must
    have been brought up to date by the re-compose itself.  (Before the fix
    tg_composite left the flag at 1 and the written env stepped with env 0's
    composite.)"""
    _cuda()
    ids = [N // 2]
    a, a0, a1 = _mass_write_run(monkeypatch, {}, ids, 1.3, True, recompose=True)
    b, b0, b1 = _mass_write_run(monkeypatch, cs.CONTROL, ids, 1.3, True, recompose=True)
    c, _, _ = _mass_write_run(monkeypatch, {}, ids, 1.3, False)
    _show("R2", A_before=a0, A_after=a1, B_before=b0, B_after=b1)
    assert a1["full"] == 0 and a1["skipped"] == 4, a1    # no simulate after the write composed
    assert b1["skipped"] == 0 and b1["full"] == 4, b1
    cs.assert_same(a, b, "R2 A vs control")
    _check_against_c(a, c, ids, "R2")


@pytest.mark.parametrize("case", ["env0", "last", "all", "empty"])
def test_gpu_r3_mass_write_id_sets(monkeypatch, case):
    """R3: R1 over the id set -- env 0 (the env whose block is shared), the
    last env (in the partial workgroup), every env with one common scale (the
    batch stays uniform: the shared cache comes back) and no env (n = 0).
    After the one compose the write costs, A skips the compose again."""
    _cuda()
    ids = {"env0": [0], "last": [N - 1], "all": list(range(N)), "empty": []}[case]
    a, a0, a1 = _mass_write_run(monkeypatch, {}, ids, 1.3, True)
    b, b0, b1 = _mass_write_run(monkeypatch, cs.CONTROL, ids, 1.3, True)
    _show("R3-" + case, A_before=a0, A_after=a1, B_before=b0, B_after=b1)
    cs.assert_same(a, b, f"R3 {case} A vs control")
    assert a0["skipped"] == 2 and a1["full"] == 1 and a1["skipped"] == 3, (a0, a1)   # skipped again afterwards
    assert b1["skipped"] == 0 and b1["full"] == 4, b1
    if case in ("env0", "last"):
        c, _, _ = _mass_write_run(monkeypatch, {}, ids, 1.3, False)
        _check_against_c(a, c, ids, "R3 " + case)


def test_gpu_r4_mass_write_and_restore(monkeypatch):
    """R4: a mass write that makes one env differ, 2 simulates, a second write
    that sets it back to 1.0, 3 simulates (2 before the first write).  The
    batch is uniform again after the restore and A goes back to the shared
    block; its states stay bit-identical to the control's."""
    _cuda()
    ids, tg = [5], cs.walk_targets(N, 7)
    out = []
    for switches in ({}, cs.CONTROL):
        sim = cs.create_under(monkeypatch, switches, lambda: cs.walk_sim(N))
        trace, marks = [], []
        for t in range(7):
            if t == 2:
                sim.set_body_mass_scale_indexed(cs.mass_rows(sim, ids, 1.3), cs.ids32(ids))
            if t == 4:
                sim.set_body_mass_scale_indexed(cs.mass_rows(sim, ids, 1.0), cs.ids32(ids))
            sim.set_dof_position_targets(tg[t])
            sim.simulate()
            trace.append(cs.snap_sim(sim))
            marks.append(cs.launch_stats(sim))
        sim.sync()
        sim.close()
        out.append((trace, marks))
    (a, ma), (b, mb) = out
    _show("R4", A=ma[-1], B=mb[-1])
    cs.assert_same(a, b, "R4 A vs control")
    # A: the first simulate and the one after each write compose, the other four skip
    assert [m["full"] for m in ma] == [1, 1, 2, 2, 3, 3, 3] and ma[-1]["skipped"] == 4, ma
    assert mb[-1]["skipped"] == 0 and mb[-1]["full"] == 7, mb[-1]


def _forces(seed=31):
    """seeded per-link force and torque tensors [N*L, 3] for the thormang model (44 links)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    f = (torch.randn(N, 44, 3, generator=g) * 15.0).to(cs.DEV).reshape(-1, 3).contiguous()
    t = (torch.randn(N, 44, 3, generator=g) * 1.5).to(cs.DEV).reshape(-1, 3).contiguous()
    return f, t


@pytest.mark.parametrize("case", ["env_skipped", "local_after_write", "torque_only", "twice", "then_body_forces"])
def test_gpu_r5_rigid_body_force_tensors(monkeypatch, case):
    """R5: apply_rigid_body_force_tensors 3 simulates into a run.

    * env_skipped: ENV space forces + torques while A skips the compose (the
      launch_rb_forces path; the control reduces inside its compose);
    * local_after_write: LOCAL space right after a property write (both reduce
      inside the compose);
    * torque_only: torques alone, compose skipped;
    * twice: two calls before one simulate, the second replaces the first
      (its forces act on the upper half of the envs only: the wrench of the
      lower half must come out exactly zero);
    * then_body_forces: apply_body_forces after it replaces the pending
      tensor (the wrench of the simulate is the given one, bit for bit, and
      nothing was reduced).

    Transplant check: after the forced simulate A's whole state is copied
    into a freshly created sim and both simulate once more; bit-identical
    results show that the forces acted for exactly one simulate and left no
    host state behind."""
    _cuda()
    from thormang_isaacgym_amd.abi import TG_PROP_STIFFNESS
    from thormang_isaacgym_amd.sim import Sim
    f, t = _forces()
    tg = cs.walk_targets(N, 6)
    upper = torch.zeros(N, 44, 3, device=cs.DEV)
    upper[N // 2:] = 1.0
    f_upper = (f.view(N, 44, 3) * upper).reshape(-1, 3).contiguous()
    out = []
    for switches in ({}, cs.CONTROL):
        sim = cs.create_under(monkeypatch, switches, lambda: cs.walk_sim(N))
        wrench = torch.randn(N, sim.G, 6, generator=torch.Generator(device="cpu").manual_seed(2)).to(cs.DEV) * 5.0
        trace = []
        for k in range(6):
            if k == 3:
                before = cs.launch_stats(sim)
                if case == "env_skipped":
                    sim.apply_rigid_body_force_tensors(f, t, Sim.ENV_SPACE)
                elif case == "local_after_write":
                    vals = sim.dof_props[TG_PROP_STIFFNESS].clone()
                    vals[7] *= 0.5
                    sim.set_dof_properties_indexed(TG_PROP_STIFFNESS, vals.contiguous(), cs.ids32([7]))
                    sim.apply_rigid_body_force_tensors(f, t, Sim.LOCAL_SPACE)
                elif case == "torque_only":
                    sim.apply_rigid_body_force_tensors(None, t, Sim.ENV_SPACE)
                elif case == "twice":
                    sim.apply_rigid_body_force_tensors(f, t, Sim.ENV_SPACE)
                    sim.apply_rigid_body_force_tensors(f_upper, None, Sim.ENV_SPACE)
                else:
                    sim.apply_rigid_body_force_tensors(f, t, Sim.ENV_SPACE)
                    sim.apply_body_forces(wrench)
            sim.set_dof_position_targets(tg[k])
            sim.simulate()
            trace.append(cs.snap_sim(sim))
            if k == 3:
                forced = cs.since(sim, before)
                applied = sim.body_force.clone()   # the group wrenches this simulate applied
                if not switches:                   # the transplant: A and a fresh sim, one simulate each
                    fresh = cs.walk_sim(N)
                    cs.transplant(sim, fresh)
                    fresh.set_dof_position_targets(tg[4])
                    fresh.simulate()
                    fresh.sync()
                    transplanted = cs.snap_sim(fresh)
                    fresh.close()
        sim.sync()
        sim.close()
        out.append((trace, forced, applied))
    (a, fa, wa), (b, fb, wb) = out
    _show("R5-" + case, A=fa, B=fb)
    cs.assert_same(a, b, f"R5 {case} A vs control")
    assert torch.equal(wa, wb), "the reduced wrenches differ between A and the control"
    cs.assert_same([a[4]], [transplanted], f"R5 {case} A vs the transplant", keys=("root_state", "dof_state"))
    reduced = {"env_skipped": ("rb_launch", "rb_in_compose"), "local_after_write": ("rb_in_compose", "rb_in_compose"),
               "torque_only": ("rb_launch", "rb_in_compose"), "twice": ("rb_launch", "rb_in_compose"),
               "then_body_forces": (None, None)}[case]
    for st, how in zip((fa, fb), reduced):
        assert st["rb_launch"] + st["rb_in_compose"] == (0 if how is None else 1), (case, st)
        assert how is None or st[how] == 1, (case, how, st)
    assert fa["skipped"] == (0 if case == "local_after_write" else 1) and fb["skipped"] == 0, (fa, fb)
    if case == "twice":
        assert float(wa[: N // 2].abs().max()) == 0.0 and float(wa[N // 2:].abs().max()) > 0.0
    elif case == "then_body_forces":
        assert torch.equal(wa, wrench)
    elif case == "torque_only":
        assert float(wa[..., :3].abs().max()) == 0.0 and float(wa[..., 3:].abs().min(2).values.max()) > 0.0
    else:
        assert float(wa.abs().min(2).values.max()) > 0.0   # (some group got a full wrench)


def test_gpu_r6_bind_state_mid_run(monkeypatch):
    """R6: after 3 simulates tg_bind_state moves dof_props, env_dirty and
    root_state to fresh tensors; one env's stiffness is then halved through
    the new props view (env_dirty set, refresh), 3 simulates follow.  The
    library must read and write the new tensors from then on."""
    _cuda()
    from thormang_isaacgym_amd.abi import TG_PROP_STIFFNESS
    env, tg = 9, cs.walk_targets(N, 6)
    out = []
    for switches, write in (({}, True), (cs.CONTROL, True), ({}, False)):
        sim = cs.create_under(monkeypatch, switches, lambda: cs.walk_sim(N))
        trace = []
        for t in range(6):
            if t == 3:
                before = cs.launch_stats(sim)
                old_root = sim.root_state
                cs.rebind(sim)
                assert torch.equal(sim.root_state, old_root)   # the live contents moved over
                if write:
                    sim.dof_props[TG_PROP_STIFFNESS, env] *= 0.5
                    sim.env_dirty[env] = 1
                sim.refresh()
            sim.set_dof_position_targets(tg[t])
            sim.simulate()
            trace.append(cs.snap_sim(sim))
        sim.sync()
        assert int(sim.env_dirty.sum()) == 0   # the compose cleared the new dirty tensor
        out.append((trace, cs.since(sim, before)))
        sim.close()
    (a, sa), (b, sb), (c, _) = out
    _show("R6", A_after=sa, B_after=sb)
    cs.assert_same(a, b, "R6 A vs control")
    assert sa["full"] == 1 and sa["skipped"] == 2 and sb["skipped"] == 0 and sb["full"] == 3, (sa, sb)
    assert cs.changed_envs(a[-1], c[-1], N) == {env}


def test_gpu_r7_exports_and_params_mid_run(monkeypatch):
    """R7: the net contact force and DOF force tensors are turned on after 3
    simulates, while A skips the compose, and off 3 simulates later; while
    they are on, tg_set_sim_params takes substeps from 1 to 2 (and back when
    they go off) and set_gravity changes gravity.  The states stay
    bit-identical to the control's and to a sim that never had the tensors
    on (the exports' contract, here mid-run); the tensors agree with the
    control's."""
    _cuda()
    tg = cs.walk_targets(N, 9)
    out = []
    for switches, tensors in (({}, True), (cs.CONTROL, True), ({}, False)):
        sim = cs.create_under(monkeypatch, switches, lambda: cs.walk_sim(N, substeps=1))

        def substeps(k):
            sp = sim.get_sim_params()
            sp.substeps = k
            sim.set_sim_params(sp)
        trace = []
        for t in range(9):
            if t == 3 and tensors:
                sim.acquire_net_contact_force_tensor()
                sim.acquire_dof_force_tensor()
            if t == 4:
                substeps(2)
            if t == 5:
                sim.set_gravity([0.3, 0.0, -9.0])
            if t == 6:
                if tensors:
                    cs.contact_tensor_off(sim)
                    cs.dof_force_tensor_off(sim)
                substeps(1)
            sim.set_dof_position_targets(tg[t])
            sim.simulate()
            trace.append(cs.snap_sim(sim))
        sim.sync()
        out.append((trace, cs.launch_stats(sim)))
        sim.close()
    (a, sa), (b, sb), (c, _) = out
    _show("R7", A=sa, B=sb)
    cs.assert_same(a, b, "R7 A vs control")
    cs.assert_same(a, c, "R7 A vs never exported", keys=("root_state", "dof_state"))
    assert sa["full"] == 1 and sa["skipped"] == 8 and sb["skipped"] == 0 and sb["full"] == 9, (sa, sb)
    on = [t for t, s in enumerate(a) if "net_contact_force" in s]
    assert on == [3, 4, 5] and all("dof_force" in a[t] for t in on), on
    assert all(float(a[t]["net_contact_force"].abs().max()) > 0 and float(a[t]["dof_force"].abs().max()) > 0
               for t in on)


def test_gpu_r8_lock_window_writes(monkeypatch):
    """R8 (model gogoro): after 3 simulates the lock window of a seat DOF is
    moved on one env through set_dof_properties_indexed (LOWER and UPPER) and
    on another through the dof_props and env_dirty views plus refresh; 4
    simulates follow.  Windows stay 1e-4 wide (TG_LOCK_WINDOW_MAX is 1e-3;
    sync would report a wider one).  Control: TG_ALWAYS_COMPOSE=1."""
    _cuda()
    from thormang_isaacgym_amd.abi import TG_PROP_LOWER, TG_PROP_UPPER
    e_api, e_view = 6, N - 2
    out = []
    for switches, write in (({}, True), ({"TG_ALWAYS_COMPOSE": "1"}, True), ({}, False)):
        sim, dni = cs.create_under(monkeypatch, switches, lambda: cs.gogoro_sim(N))
        bx, bz = dni["base_x"], dni["base_z"]
        trace = []
        for t in range(7):
            if t == 3:
                before = cs.launch_stats(sim)
            if t == 3 and write:
                for field, v in ((TG_PROP_LOWER, 0.03), (TG_PROP_UPPER, 0.0301)):
                    vals = sim.dof_props[field].clone()
                    vals[e_api, bx] = v
                    sim.set_dof_properties_indexed(field, vals.contiguous(), cs.ids32([e_api]))
                sim.dof_props[TG_PROP_LOWER, e_view, bz] = 0.02
                sim.dof_props[TG_PROP_UPPER, e_view, bz] = 0.0201
                sim.env_dirty[e_view] = 1
                sim.refresh()
            sim.simulate()
            trace.append(cs.snap_sim(sim))
        sim.sync()   # (raises if a lock window were too wide)
        out.append((trace, before, cs.since(sim, before)))
        sim.close()
    (a, a0, a1), (b, b0, b1), (c, _, _) = out
    _show("R8", A_before=a0, A_after=a1, B_before=b0, B_after=b1)
    cs.assert_same(a, b, "R8 A vs control")
    assert a0["full"] == 1 and a0["skipped"] == 2 and a1["full"] == 1 and a1["skipped"] == 3, (a0, a1)
    assert b0["skipped"] == 0 and b1["skipped"] == 0, (b0, b1)
    assert cs.changed_envs(a[-1], c[-1], N) == {e_api, e_view}


# ---------------------------------------------------------------- task rows
def _actions(n, width, steps, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [((torch.rand(n, width, generator=g) * 2 - 1) * scale).to(cs.DEV) for _ in range(steps)]


def _make(monkeypatch, switches, task, n, short, stagger=3):
    """tia.make under ``switches`` with the episode cut to ``short`` steps, so
    that timeout resets fall inside a 10-12 step run (the walk's cfg gives the
    length in seconds, episodeLength_s; the scooter tasks in steps,
    max_steps); the envs' progress counters start ``stagger`` steps apart so
    that the resets spread over the steps, not all envs at once.

    The task kernels flag an env in reset_buf at the end of one step and
    reset it in the post-physics of the next: a step *had* resets when
    reset_buf was set before it (``_pending``)."""
    import thormang_isaacgym_amd as tia
    from thormang_isaacgym_amd.cfg import load_task_cfg

    def factory():
        cfg = load_task_cfg(task, num_envs=n)
        if "max_steps" in cfg["env"]:
            cfg["env"]["max_steps"] = short
        else:
            cfg["env"]["episodeLength_s"] = short * float(cfg["sim"]["dt"]) * cfg["env"].get("controlFrequencyInv", 1)
        return tia.make(seed=11, task=task, num_envs=n, sim_device=cs.DEV, rl_device=cs.DEV, cfg=cfg)
    env = cs.create_under(monkeypatch, switches, factory)
    assert short <= int(env.max_episode_length) <= short + 1
    env.progress_buf += torch.arange(n, device=cs.DEV) % stagger
    return env


def _pending(env) -> int:
    """the envs the coming step's post-physics will reset"""
    return int(env.reset_buf.sum())


def test_gpu_t1_gogoro_mass_write_and_host_reset(monkeypatch):
    """T1: Gogoro (resets update the seat composites in place), 12 steps.
    After a step that had resets two envs get new masses; three steps later
    the host resets three envs (reset_idx).  Control: TG_ALWAYS_COMPOSE=1."""
    _cuda()
    acts = _actions(N, 1, 12, 4)
    out = []
    for switches in ({}, {"TG_ALWAYS_COMPOSE": "1"}):
        env = _make(monkeypatch, switches, "Gogoro", N, 4)
        trace, n_reset, wrote = [], 0, None
        for t in range(12):
            had = _pending(env)
            n_reset += had
            env.step(acts[t])
            trace.append(cs.snap_env(env))
            if wrote is None and t >= 2 and had > 0:   # straight after a step with resets
                assert n_reset > 0
                env.sim.set_body_mass_scale_indexed(cs.mass_rows(env.sim, [4, N - 1], 1.2), cs.ids32([4, N - 1]))
                wrote = t
            if wrote is not None and t == wrote + 3:
                env.reset_idx(torch.tensor([1, 4, N - 2], device=cs.DEV))
        env.sim.sync()
        out.append((trace, cs.launch_stats(env.sim), wrote, n_reset))
        del env
    (a, sa, wa, ra), (b, sb, wb, rb) = out
    _show("T1", A=sa, B=sb, wrote_after_step=wa, resets=ra)
    assert wa is not None and wa == wb and wa + 3 < 11 and ra == rb and ra > 0
    cs.assert_same(a, b, "T1 A vs control")
    # A composes for the creation, the mass write and the host reset only
    assert sa["full"] == 3 and sa["skipped"] == 9 and sa["list"] == 0 and sa["declined"] == 0, sa
    assert sb["skipped"] == 0 and sb["full"] == 12, sb


@pytest.mark.parametrize("case", ["plain", "prop_write", "rb_forces"])
def test_gpu_t2_gogoro_reset_list_path(monkeypatch, case):
    """T2: Gogoro with TG_SEAT_RECOMPOSE=1 in A and B (resets are listed for
    compose_list_kernel, the double-buffered reset list), 12 steps.  Straight
    after a step with resets, while the list is pending: a DOF property write
    (prop_write) or apply_rigid_body_force_tensors (rb_forces) -- the two
    branches that turn the list compose into a full one -- or nothing
    (plain).  Control: the same plus TG_ALWAYS_COMPOSE=1: A runs list
    composes, B none."""
    _cuda()
    from thormang_isaacgym_amd.abi import TG_PROP_DAMPING
    acts = _actions(N, 1, 12, 6)
    out = []
    for extra in ({}, {"TG_ALWAYS_COMPOSE": "1"}):
        env = _make(monkeypatch, dict({"TG_SEAT_RECOMPOSE": "1"}, **extra), "Gogoro", N, 4)
        sim = env.sim
        g = torch.Generator(device="cpu").manual_seed(8)
        f = (torch.randn(N, sim.L, 3, generator=g) * 20.0).to(cs.DEV).reshape(-1, 3).contiguous()
        trace, n_reset, called, delta = [], 0, None, None
        for t in range(12):
            if called is not None and t == called + 1:
                before = cs.launch_stats(sim)
            had = _pending(env)
            n_reset += had
            env.step(acts[t])
            trace.append(cs.snap_env(env))
            if called is not None and t == called + 1:
                delta = cs.since(sim, before)
            if called is None and t >= 2 and had > 0:   # this step's epilogue listed its resets: the list is pending
                assert n_reset > 0
                called = t
                if case == "prop_write":
                    vals = sim.dof_props[TG_PROP_DAMPING].clone()
                    vals[3, env.dof_name_to_id["steering_joint"]] *= 2.0
                    sim.set_dof_properties_indexed(TG_PROP_DAMPING, vals.contiguous(), cs.ids32([3]))
                elif case == "rb_forces":
                    sim.apply_rigid_body_force_tensors(f, None, sim.ENV_SPACE)
        sim.sync()
        out.append((trace, cs.launch_stats(sim), delta, called, n_reset))
        del env
    (a, sa, da, ca, ra), (b, sb, db, cb, rb) = out
    _show("T2-" + case, A=sa, B=sb, A_step_after_call=da, B_step_after_call=db, called_after_step=ca, resets=ra)
    assert ca is not None and ca == cb and ca < 11 and ra == rb and ra > 0
    cs.assert_same(a, b, f"T2 {case} A vs control")
    assert sa["list"] >= 8 and sa["skipped"] == 0 and sb["list"] == 0 and sb["skipped"] == 0 and sb["full"] == 12, \
        (sa, sb)
    # the step after the call: A's list compose, or the full one the call turned it into
    want = {"plain": dict(list=1, full=0, rb_launch=0, rb_in_compose=0),
            "prop_write": dict(list=0, full=1, rb_launch=0, rb_in_compose=0),
            "rb_forces": dict(list=0, full=1, rb_launch=0, rb_in_compose=1)}[case]
    assert all(da[k] == v for k, v in want.items()), (case, da)
    assert sa["full"] == 1 + want["full"], sa


def test_gpu_t3_walk_dr_mass_write_and_contact_tensor(monkeypatch):
    """T3: ThormangWalkDR (per-env masses and friction, pushes), 12 steps: a
    mass write on two envs before step 4, the net contact force tensor turned
    on before step 6 -- the fused step is declined while it is on -- and off
    before step 9.  Control: TG_ALWAYS_COMPOSE=1 TG_NO_SHARED_CACHE=1."""
    _cuda()
    acts = _actions(N, 33, 12, 5, scale=1.2)
    out = []
    for switches in ({}, cs.CONTROL):
        env = _make(monkeypatch, switches, "ThormangWalkDR", N, 5)
        sim = env.sim
        trace, marks, n_reset = [], [cs.launch_stats(sim)], 0
        for t in range(12):
            if t == 4:
                sim.set_body_mass_scale_indexed(cs.mass_rows(sim, [2, N - 3], 1.15), cs.ids32([2, N - 3]))
            if t == 6:
                sim.acquire_net_contact_force_tensor()
            if t == 9:
                cs.contact_tensor_off(sim)
            n_reset += _pending(env)
            env.step(acts[t])
            trace.append(cs.snap_env(env))
            marks.append(cs.launch_stats(sim))
        sim.sync()
        out.append((trace, marks, n_reset))
        del env
    (a, ma, ra), (b, mb, rb) = out
    _show("T3", A=ma[-1], B=mb[-1], resets=ra)
    assert ra == rb and ra > 0
    cs.assert_same(a, b, "T3 A vs control")
    assert [t for t, s in enumerate(a) if "net_contact_force" in s] == [6, 7, 8]
    step = [{k: ma[t + 1][k] - ma[t][k] for k in cs.STATS} for t in range(12)]
    for t, d in enumerate(step):
        if 6 <= t < 9:    # declined, then the general path: the pre-physics rides in a full compose
            assert d["declined"] > 0 and d["full"] == 1 and d["skipped"] == 0, (t, d)
        elif t in (0, 4):   # creation / the mass write
            assert d["declined"] == 0 and d["full"] == 1 and d["skipped"] == 0, (t, d)
        else:
            assert d["declined"] == 0 and d["full"] == 0 and d["skipped"] == 1, (t, d)
    assert mb[-1]["skipped"] == 0 and mb[-1]["full"] == 12, mb[-1]


def test_gpu_t4_paper_one_launch_refresh_and_host_reset(monkeypatch):
    """T4: GogoroPaper's one-launch step (16 envs: one workgroup of the
    in-launch batch sum), 10 steps, with the committed cfg's pushes on: a
    rigid-body state refresh before each of steps 4-6 (the pushes the last
    step reduced ahead become a pending tensor again) and a host reset_idx
    before step 7.  The episode
    is 10 steps, the task's push interval, and the progress counters start up
    to 5 steps apart: pushes fall on steps 3-8 and timeout resets on steps
    4-9.  Control: TG_ALWAYS_COMPOSE=1.  Windowed kernel timing (windows of 2
    step kernels with no other launch between them) shows that A ran one
    launch per step."""
    _cuda()
    n = 16
    acts = _actions(n, 1, 10, 7)
    out = []
    for switches in ({}, {"TG_ALWAYS_COMPOSE": "1"}):
        env = _make(monkeypatch, switches, "GogoroPaper", n, 10, stagger=6)
        sim = env.sim
        sim.set_kernel_timing(-2)
        trace, n_reset = [], 0
        for t in range(10):
            if t == 4:
                before = cs.launch_stats(sim)
            if t in (4, 5, 6):
                sim.refresh_rigid_body_state_tensor()
            if t == 7:
                env.reset_idx(torch.tensor([0, 5, n - 1], device=cs.DEV))
            n_reset += _pending(env)
            env.step(acts[t])
            trace.append(dict(cs.snap_env(env), pushes=env.head_perturbation.clone(),
                              pos_target=sim.dof_pos_target.clone(), vel_target=sim.dof_vel_target.clone()))
            if t == 6:
                refreshed = cs.since(sim, before)
        torch.cuda.synchronize()
        sim.set_kernel_timing(0)
        launches = sim.read_kernel_timing()[1]
        sim.sync()   # (raises if a one-launch batch sum had timed out)
        out.append((trace, cs.launch_stats(sim), refreshed, launches, n_reset, bool(env._bufs.rb_forces)))
        del env
    (a, sa, fa, la, ra, push), (b, sb, fb, lb, rb, _) = out
    _show("T4", A=sa, B=sb, A_refreshed_steps=fa, B_refreshed_steps=fb, A_windows=la, B_windows=lb, resets=ra,
          pushes=push)
    assert ra == rb and ra > 0
    cs.assert_same(a, b, "T4 A vs control")
    assert la >= 4 and lb == 0, (la, lb)
    # A composes for the creation and the host reset only
    assert sa["full"] == 2 and sa["skipped"] == 8 and sa["declined"] == 0, sa
    assert sb["skipped"] == 0 and sb["full"] == 10, sb
    if push:   # the refresh handed the reduction back to the next simulate: on its own in A, in B's compose
        assert float(torch.stack([s["pushes"] for s in a]).abs().max()) > 0.0
        assert fa["rb_launch"] == 3 and fa["rb_in_compose"] == 0 and fb["rb_in_compose"] == 3, (fa, fb)
